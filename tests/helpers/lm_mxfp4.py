"""CPU restatement of the weight-only MXFP4 format of the small-batch LM step (csrc/lm_gemv_fp4.hip, ops.quantize_blocks_mxfp4), the
hand-picked blocks its tests share, and the error bound of the GEMV on it.  Nothing here needs a GPU or a torch fp4 dtype.

Format (OCP MXFP4): e2m1 codes -- magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6} as codes 0..7, bit 3 the sign -- in blocks of 32 along K, one
power-of-two scale ``2^e`` per block stored as the byte ``e + 127``; ``e`` is the smallest integer with ``amax / 2^e <= 6``, at least
-125, 0 for an all-zero block.  6 = 0.75 * 2^3, so for ``amax = m * 2^ex`` (frexp: ``0.5 <= m < 1``) the exponent is ``ex - 3`` when
``m <= 0.75`` and ``ex - 2`` otherwise.  ``|w| / 2^e`` (exact) is rounded to the nearest magnitude, ties to the code with an even
mantissa bit (= an even code).  Codes are packed two per byte, even ``k`` in the low nibble."""
import math

import torch

from tests.helpers import lm_fp8w

U = lm_fp8w.U
C_PROLOGUE = lm_fp8w.C_PROLOGUE
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E_MIN = -125


def quant_blocks_ref(w: torch.Tensor):
    """w [N, K] (bf16 or fp32 holding bf16 values, CPU), K % 32 == 0 -> (q uint8 [N, K/2], scale uint8 [N, K/32]).  fp64 throughout:
    the division by 2^e and the distances to the two neighbouring grid points are exact there for every bf16 input."""
    wd = w.detach().cpu().double()
    N, K = wd.shape
    if K % 32:
        raise ValueError(f"K = {K} is not a multiple of 32")
    if not bool(torch.isfinite(wd).all()) or bool((wd.abs() >= 2.0 ** 120).any()):
        raise ValueError("non-finite values or magnitudes >= 2^120")
    b = wd.view(N, K // 32, 32)
    amax = b.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.75, ex - 3, ex - 2).clamp_min(E_MIN)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).long()
    t = b.abs() * torch.exp2(-e.double())[:, :, None]
    grid = torch.tensor(GRID, dtype=torch.float64)
    lo = (torch.bucketize(t, grid, right=True) - 1).clamp(0, 7)            # the largest grid point <= t
    hi = (lo + 1).clamp_max(7)
    d_lo, d_hi = t - grid[lo], grid[hi] - t
    up = (hi != lo) & ((d_hi < d_lo) | ((d_hi == d_lo) & (hi % 2 == 0)))   # nearest; a tie goes to the even code
    code = torch.where(up, hi, lo) | (torch.signbit(b).long() << 3)
    code = code.view(N, K // 2, 2)
    q = (code[:, :, 0] | (code[:, :, 1] << 4)).to(torch.uint8)
    return q, (e + 127).to(torch.uint8)


def codes_of(q: torch.Tensor) -> torch.Tensor:
    """q uint8 [N, K/2] -> the 4-bit codes in k order, int64 [N, K]."""
    q = q.cpu().long()
    return torch.stack((q & 0xF, q >> 4), dim=-1).view(q.shape[0], -1)


def code_value(codes: torch.Tensor) -> torch.Tensor:
    """fp64 value of e2m1 codes 0..15."""
    mag = torch.tensor(GRID, dtype=torch.float64)[codes & 7]
    return torch.where(codes >= 8, -mag, mag)


def dequant_ref(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp64 values [N, K] of (q, scale): exact.  (One table lookup per byte: the two values it holds.)"""
    byte = torch.arange(256)
    table = code_value(torch.stack((byte & 0xF, byte >> 4), dim=-1))        # [256, 2]
    N = q.shape[0]
    v = table[q.cpu().long()].view(N, -1, 32)
    v *= torch.exp2(scale.cpu().double() - 127.0)[:, :, None]
    return v.view(N, -1)


def is_exactly_bf16(v64: torch.Tensor) -> bool:
    return bool(torch.isfinite(v64).all()) and bool(torch.equal(v64.float().bfloat16().double(), v64))


LAYER_MATRICES = ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "gating.linear_in.weight", "gating.linear_out.weight")


def quantise_state_dict(sd: dict, cfg: dict):
    """The state dict LMModel.quantize_weights_("mxfp4") leaves behind (host restatement): the four per-layer matrices of the temporal
    stack replaced by their MXFP4-dequantised values (fp8 rows where K is no multiple of 32), text_linear and the depformer_in[k] by
    their fp8-dequantised values (helpers.lm_fp8w), everything else untouched.  Returns (state dict, names as MXFP4, names as fp8)."""
    layer = [f"transformer.layers.{l}.{n}" for l in range(cfg["num_layers"]) for n in LAYER_MATRICES]
    heads = ["text_linear.weight"] + [f"depformer_in.{k}.weight" for k in range(cfg["dep_q"])]
    out, as4, as8 = dict(sd), [], list(heads)
    for name in layer:
        if sd[name].shape[1] % 32 == 0:
            q, s = quant_blocks_ref(sd[name])
            out[name] = dequant_ref(q, s).to(sd[name].dtype)
            as4.append(name)
        else:
            as8.append(name)
    for name in as8:
        q, s = lm_fp8w.quant_rows_ref(sd[name])
        out[name] = lm_fp8w.dequant_ref(q, s).to(sd[name].dtype)
    return out, as4, as8


# ---- hand-picked blocks: (32 bf16-representable values, expected exponent e, expected codes of the leading elements)
def special_blocks():
    """[blocks, 32] fp32 (all values bf16-representable), the expected exponent of every block, and {block: leading expected codes}."""
    rows, exps, want = [], [], {}

    def add(vals, e, codes):
        r = torch.zeros(32)
        r[:len(vals)] = torch.tensor(vals, dtype=torch.float64).float()
        assert torch.equal(r.bfloat16().float(), r), vals
        want[len(rows)] = codes
        rows.append(r)
        exps.append(e)

    add([], 0, [0] * 32)                                                                  # all-zero block: e = 0, zero codes
    # amax = 6 exactly lands on e = 0: every tie of the grid (0.25 1.25 2.5 5 down to the even code, 0.75 1.75 3.5 up), both signs,
    # +-0, and every grid point itself
    add([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -5.0, 0.0, -0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, -0.75, -1.25, -1.75, -2.5,
         -3.5, -6.0, 0.2490234375, 0.251953125, 5.03125],
        0, [7, 0, 2, 2, 4, 4, 6, 6, 8, 0xE, 0, 8, 1, 2, 3, 4, 5, 6, 0xA, 0xA, 0xC, 0xC, 0xE, 0xF, 0, 1, 7])
    add([6.0 * 2.0 ** -9, 1.25 * 2.0 ** -9, 2.0 ** -9], -9, [7, 2, 2])                    # amax = 6 * 2^-9 exactly
    add([6.03125, 1.0, 2.5, -3.0], 1, [5, 1, 2, 0xB])                                      # one bf16 ulp above 6: the next exponent
    add([6.03125 * 2.0 ** -9, 2.0 ** -9], -8, [5, 1])
    add([-6.0 * 2.0 ** 20, 2.0 ** 20, 3.0 * 2.0 ** 20], 20, [0xF, 2, 5])                   # a negative amax, large scale
    # bf16 subnormals (multiples of 2^-133): amax = 1.5 * 2^-127 asks for e = -129, the clamp gives -125 and smaller codes
    add([2.0 ** -127, 1.5 * 2.0 ** -127, 2.0 ** -133, -1.5 * 2.0 ** -127], E_MIN, [0, 1, 0, 9])
    add([2.0 ** -126 * 1.5, 2.0 ** -126], E_MIN, [2, 1])                                   # normal, still at the clamp (e = -128 asked)
    add([1.9921875 * 2.0 ** 119, 2.0 ** 118, -2.0 ** 117], 118, [6, 2, 9])                # amax just below 2^120
    return torch.stack(rows), torch.tensor(exps), want


# ---- bound of rst_gemv_mxfp4w_f32 ------------------------------------------------------------------------------------------------------
def c_gemv(K: int) -> int:
    """Backward-error constant of one output of the MXFP4 GEMV, in units of 2^-24 of sum_k |w_k x_k| (+ |bias| + |res|).

    The convert yields code * 2^e, a normal number with two significant bits: exact.  The product inside an fma is exact, so every
    rounding is an addition's:
      * a lane owns 32 consecutive k of every 2048-wide chunk and adds them as two chains (even / odd k) of 16 packed FMAs each,
        joined by one addition per chunk, the joined sum being the even chain's start in the next chunk: 17 * ceil(K / 2048) roundings
        at most along any path;
      * the 64 lanes meet in a butterfly of 6 additions (the DPP form: 4 within a row of 16 lanes, 2 across the four rows);
      * the block scales are part of the weights (nothing is multiplied afterwards), the bias and the residual are one addition each: 2.
    With n = 17 * ceil(K / 2048) + 8 roundings the error is at most gamma_n = n u / (1 - n u) times the sum of magnitudes; one more
    unit covers the denominator (n u < 2^-16)."""
    return 17 * math.ceil(K / 2048) + 8 + 1
