"""The adapter-bank launches (csrc/lm_lora_bank.hip behind ops.lora_bank_shrink / ops.lora_bank_expand) restated for their tests:
the model-level fixtures (one base, three adapter sets), operands, an fp32 emulation in plain torch, fp64 references and the
per-element error bounds.  Nothing here needs a GPU; tests/test_lora_bank_cpu.py checks the bounds against the emulation and against
four planted defects.

Bounds, in units of U = 2^-24 of the sum of magnitudes, from the kernels' schedule:

  shrink, a = post_scale * sum_k A_k P(x)_k.  The bf16 weight is widened exactly and the product inside an fmaf is not rounded, so every
  rounding is an addition's.  A lane multiplies 8 consecutive k of every 512-wide chunk into ONE fmaf chain: 8 * ceil(K / 512)
  roundings; the 64 lanes meet in a butterfly of 6 additions; the multiplication by post_scale is one more.  n = 8 * ceil(K / 512) + 7
  roundings give gamma_n = n u / (1 - n u); one more unit covers the denominator:
      c_shrink(K) = 8 * ceil(K / 512) + 8,
  and a prologue adds C_PROLOGUE (helpers.lm_fp8w: the fp32 error of RMSNorm / SiLU gate relative to |P(x)|, the same arithmetic as the
  GEMV's prologues) on the same sum:
      |a - a64| <= (c_shrink(K) + C_PROLOGUE [prologue != 0]) * U * |post_scale| * sum_k |A_k P(x)_k|     (+ the gate's flush term).

  expand, y' = y + sum_j B_j a_j.  ONE fmaf chain over the r' columns started at zero: r' roundings (the first addition to zero is exact,
  which is not used); then one addition into y, whose rounding is at most U |y'| <= U (|y| + |sum|).  Charging that last rounding's
  |sum| part to the chain and one unit to the denominator:
      c_expand(r') = r' + 2,
      |y' - y64| <= c_expand(r') * U * sum_j |B_j| (|a_j| + da_j) + sum_j |B_j| da_j + U |y|,
  with da_j the bound on the error of the a_j fed in (zero when expand is tested on its own).
A base-model row (id outside [0, n_adapters)) has no tolerance: a = 0, y' = y bit for bit."""
import math

import torch
import torch.nn.functional as F

from rstnet_amd import synth
from tests.helpers import gemv_bounds as GB
from tests.helpers.lm_fp8w import C_PROLOGUE, U

# ---- model-level fixtures: ONE base (that of seed 21), the adapter tensors of seeds 21 / 22 / 23 -------------------------------------
SET_SEEDS = (21, 22, 23)
CFGS = {"gqa": dict(synth.GPT_TINY_GQA), "mha": dict(synth.GPT_TINY_MHA),
        "gqa_qkv_alpha6": {**synth.GPT_TINY_GQA, "lora_alpha": 6, "lora_key": True}}      # q, k, v adapted; alpha / r not a power of two


def is_lora(k: str) -> bool:
    return k.endswith((".lora_A", ".lora_B"))


def base_sd(cfg_d: dict) -> dict:
    return {k: v for k, v in synth.gpt_state_dict(cfg_d, SET_SEEDS[0]).items() if not is_lora(k)}


def adapter_sets(cfg_d: dict) -> list:
    return [{k: v for k, v in synth.gpt_state_dict(cfg_d, s).items() if is_lora(k)} for s in SET_SEEDS]


# ---- ops-level operands ----------------------------------------------------------------------------------------------------------------
def bank_operands(n_adapters: int, r: int, K: int, N: int, seed: int = 0):
    """(A_bank bf16 [n, r, K], B_bank bf16 [n, N, r]): adapter i scaled by 16^i (a row that reads its neighbour's adapter is off by an
    order of magnitude), rows inside an adapter spanning 2^-4 .. 2^4."""
    g = torch.Generator().manual_seed(1000 + seed)
    A = torch.stack([GB.mixed_rows(r, K, g, -4, 4) * 16.0 ** i / K ** 0.5 for i in range(n_adapters)]).bfloat16()
    B = torch.stack([GB.mixed_rows(N, r, g, -4, 4) * 16.0 ** i / r ** 0.5 for i in range(n_adapters)]).bfloat16()
    return A, B


def row_ids(ids: torch.Tensor, rows: int, rows_per_id: int) -> torch.Tensor:
    return ids.long().repeat_interleave(rows_per_id)[:rows]


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------
def c_shrink(K: int) -> int:
    return 8 * math.ceil(K / 512) + 8


def c_expand(r: int) -> int:
    return r + 2


def shrink_ref(x, A_bank, ids, rows_per_id=1, prologue=0, alpha=None, eps=GB.EPS_RMS, post_scale=1.0):
    """(a64 [rows, r], bound) of the shrink launch; base-model rows: zeros with a zero bound."""
    n_ad, r, K = A_bank.shape
    rid = row_ids(ids, x.shape[0], rows_per_id)
    P = GB.p_ref(x.double(), K, prologue, None if alpha is None else alpha.double(), eps)
    a = torch.zeros(x.shape[0], r, dtype=torch.float64)
    bound = torch.zeros_like(a)
    c = (c_shrink(K) + (C_PROLOGUE if prologue else 0)) * U
    for i in range(n_ad):                                                 # (rows of one adapter at a time: no [rows, r, K] gather)
        sel = rid == i
        A = A_bank[i].double()
        a[sel] = P[sel] @ A.t() * post_scale
        bound[sel] = c * (P[sel].abs() @ A.abs().t()) * abs(post_scale)
        if prologue == 2:       # the fp32 silu(u) is -0 where expf(-u) overflows (helpers.gemv_bounds.reference_bf16)
            bound[sel] += (x[sel][:, K:].double().abs() * 2.0 ** -120) @ A.abs().t() * abs(post_scale)
    return a, bound


def expand_ref(a, B_bank, ids, y, rows_per_id=1, da=None):
    """(y64 [rows, N], bound) of the expand launch on the fp32 ``a`` it is fed (``da``: the bound on that input's own error, when the
    reference is carried through from the shrink); base-model rows: ``y`` itself with a zero bound."""
    n_ad, N, r = B_bank.shape
    rid = row_ids(ids, a.shape[0], rows_per_id)
    a64 = a.double()
    da = torch.zeros_like(a64) if da is None else da
    y64 = y.double().clone()
    bound = torch.zeros_like(y64)
    for i in range(n_ad):
        sel = rid == i
        Bm = B_bank[i].double()
        y64[sel] += a64[sel] @ Bm.t()
        bound[sel] = c_expand(r) * U * ((a64[sel].abs() + da[sel]) @ Bm.abs().t()) + da[sel] @ Bm.abs().t() + U * y[sel].double().abs()
    return y64, bound


# ---- fp32 emulation of the two launches in plain torch (no schedule: what any correct fp32 implementation computes) ---------------------
def emul_shrink(x, A_bank, ids, rows_per_id=1, prologue=0, alpha=None, eps=GB.EPS_RMS, post_scale=1.0, *, neighbour=False,
                skip_prologue=False, no_post_scale=False):
    """fp32 ``[rows, r]``.  Planted defects: ``neighbour`` (row 1 reads the adapter of row 0's id + 1), ``skip_prologue`` (x as it is, the
    first K columns), ``no_post_scale``."""
    n_ad, r, K = A_bank.shape
    rid = row_ids(ids, x.shape[0], rows_per_id)
    ok = (rid >= 0) & (rid < n_ad)
    if neighbour:
        rid = rid.clone()
        rid[1] = (rid[1] + 1) % n_ad
    if skip_prologue or prologue == 0:
        P = x[:, :K]
    elif prologue == 1:
        P = x * (alpha * torch.rsqrt(torch.tensor(eps, dtype=torch.float32) + (x * x).mean(dim=1, keepdim=True)))
    else:
        P = F.silu(x[:, :K]) * x[:, K:]
    a = torch.einsum("brk,bk->br", A_bank.float()[rid.clamp(0, n_ad - 1)], P.float())
    if not no_post_scale:
        a = a * post_scale
    return a * ok[:, None].float()


def emul_expand(a, B_bank, ids, y, rows_per_id=1, *, neighbour=False, drop_last_block=False):
    """fp32 ``[rows, N]``.  Planted defects: ``neighbour`` (row 1 reads another adapter), ``drop_last_block`` (the last 16 rank columns)."""
    n_ad, N, r = B_bank.shape
    rid = row_ids(ids, a.shape[0], rows_per_id)
    ok = (rid >= 0) & (rid < n_ad)
    if neighbour:
        rid = rid.clone()
        rid[1] = (rid[1] + 1) % n_ad
    rr = r - 16 if drop_last_block else r
    s = torch.einsum("bnr,br->bn", B_bank.float()[rid.clamp(0, n_ad - 1)][:, :, :rr], a[:, :rr])
    return torch.where(ok[:, None], y + s, y)


def worst(got, ref, bound) -> float:
    """max over elements of |got - ref| / bound (0 / 0 = 0, x / 0 = inf)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())
