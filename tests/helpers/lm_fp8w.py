"""CPU restatement of the weight-only fp8 format of the small-batch LM step (csrc/lm_gemv_fp8.hip, ops.quantize_rows_fp8), the
hand-picked rows its tests share, and the error bounds of the GEMV on it.  Nothing here needs a GPU.

Format: OCP e4m3fn bytes ``q [N, K]`` and one fp32 scale per row, a power of two ``2^e`` with ``e`` the smallest integer such that
``amax / 2^e <= 448``; ``q = RNE_e4m3(w / 2^e)``.  448 = 0.875 * 2^9, so for ``amax = m * 2^ex`` (frexp: ``0.5 <= m < 1``) the exponent
is ``ex - 9`` when ``m <= 0.875`` and ``ex - 8`` otherwise; an all-zero row takes ``e = 0``."""
import math

import torch

U = 2.0 ** -24
# fp32 error of the activation prologues relative to |P(x)| in units of 2^-24, as tests/test_lm_operands_gpu.py states and derives it
# (RMSNorm: <= 16, SiLU gate: <= 6; both held to 32)
C_PROLOGUE = 32


def quant_rows_ref(w: torch.Tensor):
    """w [N, K] (bf16 or fp32 holding bf16 values, CPU) -> (q uint8 [N, K], scale fp32 [N]).  The division by the scale is done in
    fp64, where it is exact for every bf16 input and every scale; the rounding is torch's float8_e4m3fn conversion (round to nearest
    even, e4m3 subnormals)."""
    wd = w.detach().cpu().double()
    amax = wd.abs().amax(dim=1)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).long()
    t = (wd * torch.exp2(-e.double())[:, None]).float()        # |t| <= 448; anything inexact in fp32 is below 2^-126 and rounds to +-0
    q = t.to(torch.float8_e4m3fn).view(torch.uint8)
    return q, torch.exp2(e.double()).float()


def fp8_value(q: torch.Tensor) -> torch.Tensor:
    return q.view(torch.float8_e4m3fn).double()


def dequant_ref(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp64 values of (q, scale): exact."""
    return fp8_value(q.cpu()) * scale.cpu().double()[:, None]


def is_exactly_bf16(v64: torch.Tensor) -> bool:
    return bool(torch.equal(v64.float().bfloat16().double(), v64))


def quantise_state_dict(sd: dict, cfg: dict) -> dict:
    """The state dict of the fp8-rounded model: every matrix LMModel.quantize_weights_ covers replaced by its dequantised values (host
    restatement), everything else untouched.  CPU tensors in, same dtypes out."""
    covered = [f"transformer.layers.{l}.{n}" for l in range(cfg["num_layers"])
               for n in ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "gating.linear_in.weight", "gating.linear_out.weight")]
    covered += ["text_linear.weight"] + [f"depformer_in.{k}.weight" for k in range(cfg["dep_q"])]
    out = dict(sd)
    for name in covered:
        q, s = quant_rows_ref(sd[name])
        out[name] = dequant_ref(q, s).to(sd[name].dtype)
    return out, covered


# ---- hand-picked rows: (row of bf16-representable values, expected exponent e, expected bytes of the leading elements or None)
def special_rows(K: int = 32):
    """[rows, K] fp32 (all values bf16-representable), the expected exponent of every row, and {row: leading expected bytes}."""
    rows, exps, want = [], [], {}

    def add(vals, e, codes=None):
        r = torch.zeros(K)
        r[:len(vals)] = torch.tensor(vals, dtype=torch.float64).float()
        assert torch.equal(r.bfloat16().float(), r), vals
        if codes is not None:
            want[len(rows)] = codes
        rows.append(r)
        exps.append(e)

    add([], 0, [0] * 4)                                                                   # all-zero row: e = 0, zero bytes
    # scale 1 (amax = 448 exactly lands on e = 0): RNE ties in both directions, e4m3 subnormals and their ties, values below half
    # the smallest subnormal (2^-10), +-0
    add([448.0, 1.0625, 1.1875, -1.0625, -1.1875, 3 * 2.0 ** -10, 2.0 ** -10, 2.0 ** -11, -2.0 ** -11, 7 * 2.0 ** -10, 5 * 2.0 ** -10,
         2.0 ** -9, -2.0 ** -9, 0.0, -0.0, 2.0 ** -6, 2.0 ** -6 - 2.0 ** -10, 3 * 2.0 ** -11, 416.0 + 16.0, 240.0, 1.0],
        0, [0x7E, 0x38, 0x3A, 0xB8, 0xBA, 0x02, 0x00, 0x00, 0x80, 0x04, 0x02, 0x01, 0x81, 0x00, 0x80, 0x08, 0x08, 0x01, 0x7E, 0x77, 0x38])
    add([448.0 * 2.0 ** -9, 2.0 ** -9 * 1.0625], -9, [0x7E, 0x38])                       # amax = 448 * 2^-9 exactly
    add([(448.0 + 2.0) * 2.0 ** -9, 2.0 ** -9 * 1.0625], -8, [0x76, 0x30])                # one bf16 ulp above: the next exponent
    add([-448.0 * 2.0 ** 20, 2.0 ** 20], 20, [0xFE, 0x38])                                # a negative amax, large scale
    add([2.0 ** 3] + [2.0 ** -(i % 21) * (1 + (i % 5) / 8) for i in range(K - 1)], -5)    # a row spanning 2^-20 .. 2^3
    add([2.0 ** -100 * 1.5, -2.0 ** -110], -108)                                          # tiny magnitudes: scale far below 1
    add([2.0 ** -133, 3 * 2.0 ** -133], -140, [0x70, 0x7C])                               # bf16 subnormals: scale is an fp32 subnormal
    return torch.stack(rows), torch.tensor(exps), want


# ---- bounds of rst_gemv_fp8w_f32 --------------------------------------------------------------------------------------------------------
def c_gemv(K: int) -> int:
    """Backward-error constant of one output of the fp8 GEMV, in units of 2^-24 of sum_k |w_k x_k| (+ |bias| + |res|).

    The decoded weight (e4m3 -> fp32) and the product inside an fmaf are exact, so every rounding is an addition's:
      * a lane owns 16 consecutive k of every 1024-wide chunk and adds them with ONE fmaf chain: 16 * ceil(K / 1024) roundings at most
        (the K-split schedule gives a lane only every fourth chunk: shorter);
      * the 64 lanes meet in a butterfly of 6 additions; the K-split schedule then adds its four waves' partial sums: 3 more;
      * the row scale is a power of two (exact), the bias and the residual are one addition each: 2.
    With n = 16 * ceil(K / 1024) + 11 roundings the error is at most gamma_n = n u / (1 - n u) times the sum of magnitudes; one more unit
    covers the denominator (n u < 2^-16)."""
    return 16 * math.ceil(K / 1024) + 11 + 1
