"""The default one-to-four-row GEMVs (csrc/lm_step.hip: bf16 weights behind ops.gemv_bf16, fp32 weights behind ops.linear at M <= 4)
restated for their tests: which kernel instance rst_launch_gemv picks (`route`), the case tables of tests/test_gemv_bounds_gpu.py,
operands, fp64 references and per-element error bounds.  Nothing here needs a GPU; tests/test_gemv_bounds_cpu.py checks the tables
against `route` and the bounds against plain fp32 torch and three emulated defects."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import codec_streams as CS
from tests.helpers import lm_fp8w as Q

U = Q.U
EPS_RMS = 1e-8
EPS_LN = 1e-5
ACT_GELU = 1
GEMV_WAVES = 4
LDS_FLOATS = 32768                   # lm_step.hip:532-533: B * K floats of activation stage at most


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def mixed_rows(rows, cols, g, lo=-20, hi=20):
    """randn rows scaled by 2^e, e uniform in [lo, hi] (row 0 at the low end, the last row at the high end: every tile mixes them)."""
    e = torch.randint(lo, hi + 1, (rows,), generator=g)
    e[0], e[-1] = lo, hi
    return torch.randn(rows, cols, generator=g) * torch.exp2(e.double()).float()[:, None]


def p_ref(x64, K, mode, alpha64=None, eps=EPS_RMS):
    """fp64 activation prologue of the LM GEMVs: 0 none, 1 RMSNorm (eps as the fp32 number the kernel adds), 2 SiLU gate of [u | v]."""
    if mode == 1:
        e = float(np.float32(eps))
        return x64 * alpha64 / torch.sqrt(e + (x64 * x64).mean(dim=1, keepdim=True))
    if mode == 2:
        u, v = x64[:, :K], x64[:, K:]
        return F.silu(u) * v
    return x64


# ---- the dispatch -----------------------------------------------------------------------------------------------------------------------
def cap_grid(g: int, cap: int) -> int:
    """csrc/lm_common.h cap_grid: at least one workgroup, at most `cap` (no ceiling of its own beyond the caller's)."""
    return 1 if g < 1 else min(g, cap)


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def route(B, N, K, prologue=0, gate_out=False, w_f32=False, act_out=0):
    """The kernel instance rst_launch_gemv picks and its launch facts: a plain restatement of csrc/lm_step.hip:535-585.

      * rpw4 (line 536): four rows per wave for bf16 weights without gate_out when ceil(N / 16) >= 512, i.e. N >= 8177;
      * norm_stream (538): bf16, B = 1, RMSNorm, K <= 4096, no activation, N * K >= 2^24 -> gemv_norm_kernel<gate_out> (565-567);
      * fp32 weights (551-558) always take gemv_kernel<B, 2, true>;
      * the K-split schedule (570-573): bf16, B = 1, no prologue / activation / gate_out, N * K >= 2^24, K >= 2048;
      * everything else (575-584): gemv_kernel<B, 4 or 2, false>;
      * the grid (539-541): cap_grid(launch groups, 1024 for norm_stream, else 512 when B * K * 4 > 48 KiB, else 768); the K-split
        launch has cap_grid(ceil(N / 8), 1024) (571-572).
    `groups` is the trip count of the kernel's own row-group loop (gemv_kernel: ceil(N / (RPW * 4)) or ceil(N / 2 / 4) with gate_out;
    gemv_norm_kernel always has RPW = 2, so with rpw4 it runs twice the groups the launcher sized the grid for; K-split: ceil(N / 8)).
    `strided`: some workgroup runs more than one group (the path that re-reads residual / re-issues the prefetch); `ragged`: the last
    group has fewer rows than a full one."""
    assert 1 <= B <= 4 and K % 8 == 0 and B * K <= LDS_FLOATS and prologue in (0, 1, 2, 3)
    assert not gate_out or (N % 2 == 0 and not w_f32 and not act_out)
    rpw4 = not w_f32 and not gate_out and prologue < 4 and _cdiv(N, 16) >= 512
    norm_stream = not w_f32 and B == 1 and prologue == 1 and K <= 4096 and not act_out and N * K >= 1 << 24
    lds = B * K * 4
    rows_per_group = (4 if rpw4 else 2) * GEMV_WAVES
    launch_groups = _cdiv(N // 2, GEMV_WAVES) if gate_out else _cdiv(N, rows_per_group)
    grid = cap_grid(launch_groups, 1024 if norm_stream else (512 if lds > 48 * 1024 else 768))
    groups, rows = launch_groups, (GEMV_WAVES if gate_out else rows_per_group)
    total = N // 2 if gate_out else N
    if w_f32:
        name, family = f"gemv<{B},2,f32>", "gemv_f32"
    elif norm_stream:
        name = family = "norm_gate" if gate_out else "norm"
        rows = GEMV_WAVES if gate_out else 2 * GEMV_WAVES
        groups = _cdiv(total, rows)
    elif B == 1 and prologue == 0 and not act_out and not gate_out and N * K >= 1 << 24 and K >= 2048:
        name = family = "ksplit"
        rows = 8
        groups = _cdiv(N, 8)
        grid = cap_grid(groups, 1024)
    else:
        name, family = f"gemv<{B},{4 if rpw4 else 2}>", "gemv"
    return dict(name=name, family=family, groups=groups, grid=grid, strided=groups > grid, ragged=total % rows != 0, lds=lds)


# ---- the case tables --------------------------------------------------------------------------------------------------------------------
# bf16: (purpose, N, K, batch sizes, [(prologue, res, bias, gate_out), ...]); every B is crossed with every switch tuple.
# N * K of the cases a 2^24 threshold forces stays below 1.3 * 2^24 (one 32 .. 40 MB weight, one launch).
_ROWS_BF16 = [
    ("rpw4, ragged last group (8179 = 511 * 16 + 3)", 8179, 64, (1, 2, 3, 4), [(0, 1, 1, 0), (1, 0, 0, 0), (2, 1, 0, 0)]),
    ("rpw4 grid-strided, residual on later groups (769 groups)", 12301, 64, (2, 4), [(0, 1, 1, 0)]),
    ("rpw2 grid-strided (769 groups > 768)", 6151, 64, (1, 3), [(0, 1, 0, 0), (1, 0, 1, 0)]),
    ("rpw2, 64 KB stage -> grid 512, strided (513 groups)", 4100, 4096, (4,), [(0, 1, 1, 0)]),
    ("norm, exactly at the 2^24 threshold", 4096, 4096, (1,), [(1, 0, 0, 0), (1, 1, 1, 0)]),
    ("just under it -> gemv<1,2>", 4095, 4096, (1,), [(1, 1, 1, 0)]),
    ("norm, K tail (5 chunks, the last one lane wide), ragged + strided", 8203, 2056, (1,), [(1, 1, 1, 0)]),
    ("norm_gate, ragged + strided (half = 4101)", 8202, 2048, (1,), [(1, 0, 1, 1), (1, 0, 0, 1)]),
    ("ksplit, one chunk per wave", 8192, 2048, (1,), [(0, 0, 0, 0), (0, 1, 1, 0)]),
    ("ksplit, 5 chunks (2/1/1/1), tail lane, ragged + strided (1026 groups)", 8201, 2056, (1,), [(0, 1, 1, 0)]),
    ("ksplit, 9 chunks (3/2/2/2), tail lane, ragged", 4093, 4104, (1,), [(0, 1, 1, 0)]),
    ("ksplit, 22 chunks (6/6/5/5)", 1490, 11264, (1,), [(0, 1, 0, 0)]),
    ("gate_out in gemv_kernel, strided (half = 3075)", 6150, 64, (2, 3, 4), [(1, 0, 1, 1), (0, 0, 0, 1)]),
    ("gate_out, tiny", 10, 16, (2, 4), [(1, 0, 1, 1)]),
    ("RMSNorm re-read loop (K > 4096)", 37, 11264, (2,), [(1, 1, 0, 0)]),
    ("one element past the register-resident range", 37, 4104, (1, 2), [(1, 0, 0, 0)]),
    ("B * K = 32768 exactly", 33, 8192, (4,), [(0, 1, 0, 0)]),
    ("B * K = 32768 exactly", 33, 16384, (2,), [(0, 1, 0, 0), (2, 0, 0, 0)]),
    ("B * K = 32768 exactly", 9, 32768, (1,), [(0, 1, 0, 0), (2, 0, 0, 0)]),
    ("divergent tail (some lanes take the two-chunk loop, others the single chunk)", 37, 1032, (1, 3), [(0, 0, 1, 0), (2, 0, 0, 0)]),
    ("prefetch plus an 8-wide tail", 5, 520, (1, 4), [(0, 1, 1, 0)]),
    ("a single lane", 5, 8, (1, 4), [(0, 1, 1, 0)]),
]
# (B, N, K, prologue, res, bias, gate_out)
CASES_BF16 = [(B, N, K, m, bool(r), bool(b), bool(g)) for _, N, K, Bs, sw in _ROWS_BF16 for B in Bs for m, r, b, g in sw]

# fp32: (purpose, Ms, K, N, [(ln, bias, gelu, res, scale), ...], LayerNorm rows planted)
_ROWS_F32 = [
    ("codec in-projection", (1, 2, 4), 512, 1536, [(1, 1, 0, 0, 0)], True),
    ("codec FFN in", (1, 2, 3, 4), 512, 2048, [(1, 0, 1, 0, 0), (1, 1, 1, 0, 0)], True),
    ("codec FFN out / out-projection", (1, 2, 4), 2048, 512, [(0, 0, 0, 1, 1), (0, 1, 0, 1, 1)], True),
    ("64 KB stage, grid 512, strided, residual on later groups", (4,), 4096, 4100, [(0, 1, 0, 1, 1)], False),
    ("strided at grid 768", (1,), 64, 6151, [(1, 0, 1, 1, 1)], False),
    ("M * K = 32768", (4,), 8192, 24, [(1, 0, 0, 0, 0)], False),
    ("M * K = 32768", (1,), 32768, 9, [(0, 0, 0, 0, 0)], False),
    ("smallest", (1, 3), 8, 1, [(1, 1, 0, 0, 0)], False),
]
# (M, K, N, ln, bias, gelu, res, scale, special rows)
CASES_F32 = [(M, K, N, bool(l), bool(b), bool(a), bool(r), bool(s), sp) for _, Ms, K, N, sw, sp in _ROWS_F32 for M in Ms
             for l, b, a, r, s in sw]


def route_bf16(case):
    B, N, K, mode, res, bias, gate = case
    return route(B, N, K, mode, gate)


def route_f32(case):
    M, K, N, ln, bias, gelu = case[:6]
    return route(M, N, K, 3 if ln else 0, False, True, ACT_GELU if gelu else 0)


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------
def c_gemv(K: int) -> int:
    """helpers.lm_fp8w.c_gemv(K) = 16 * ceil(K / 1024) + 12, in units of 2^-24 of sum_k |w_k x_k| + |bias| + |res|.  Its derivation holds
    for the three bf16 schedules and for fp32 weights alike; walking the loops of csrc/lm_step.hip once:

      * the product inside an fmaf is not rounded (bf16 x fp32 and fp32 x fp32 alike), so every rounding is an addition's;
      * gemv_kernel: a lane multiplies 8 consecutive k of every 512-wide chunk (the prefetched chunk, then pairs of chunks, then one
        tail chunk) into ONE fmaf chain per (row, batch row): 8 * ceil(K / 512) <= 16 * ceil(K / 1024) roundings;
      * gemv_norm_kernel: the same 8 per 512-chunk over at most 8 chunks (K <= 4096);
      * gemv_ksplit_kernel: a wave takes every fourth chunk only, 8 * ceil(ceil(K / 512) / 4) roundings: shorter;
      * wave_sum: a butterfly of 6 additions; the K-split schedule then adds the four waves' partial sums in wave order: 3 more;
      * bias and residual: one addition each (the fp32 route's GELU and LayerScale are charged to the epilogue's magnitude,
        codec_streams.epilogue64).
    n = 16 * ceil(K / 1024) + 11 roundings give gamma_n = n u / (1 - n u); one more unit covers the denominator."""
    return Q.c_gemv(K)


def c_ln(K: int):
    """Error constants (c_hat, c_mean) of the LayerNorm prologue (gemv_kernel, prologue 3), in units of 2^-24 per staged element: c_hat
    of |x_hat gamma| + |beta| (codec_streams.layernorm64's magnitude), c_mean of the mean term rstd |gamma| mean|x|.  The kernel makes
    two passes, each a per-thread chain of ceil(K / 256) additions (256 threads), a 6-step butterfly and 3 cross-wave additions:
    n_pass = ceil(K / 256) + 9.

      * mean: n_pass roundings and the division by K, relative to mean|x|: an error of (n_pass + 1) u mean|x| in the mean moves
        every x - mean by that much, and the output by rstd |gamma| times it -- the mean term.  (Its effect on the variance is of
        second order: the deviations from the true mean sum to zero.)  c_mean = n_pass + 1, plus one unit for the second order.
      * variance: d = x - mean is rounded once (twice in d^2), the sum of the positive d^2 takes n_pass roundings, then / K and + eps:
        n_pass + 4 inside the square root, so half of that on rstd, plus the square root and the reciprocal: n_pass / 2 + 4;
      * the staged value (x - mean) * rstd * gamma + beta: the subtraction, two multiplications, one addition: 4.
        c_hat = ceil(n_pass / 2) + 8, plus one unit for the second order."""
    n_pass = math.ceil(K / 256) + 9
    return math.ceil(n_pass / 2) + 8 + 1, n_pass + 1 + 1


def gate_carry(h, dh):
    """silu(u) * v of h = [u | v] (fp64) and the bound on its error when h is off by at most dh: first order in the derivative
    (|silu'| < 1.1) with the product term, 8 roundings for the fp32 silu and the product, and the fp32 silu's flush to zero where
    expf(-u) overflows (|silu(u)| < 2^-119 there)."""
    I = h.shape[1] // 2
    u, v, du, dv = h[:, :I], h[:, I:], dh[:, :I], dh[:, I:]
    ref = F.silu(u) * v
    bound = 1.1 * (v.abs() + dv) * du + F.silu(u).abs() * dv + 8 * U * ref.abs() + v.abs() * 2.0 ** -110
    return ref, bound


# ---- bf16 weights: ops.gemv_bf16 --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _weight_bf16(N, K):
    g = torch.Generator().manual_seed(7 * N + K)
    w = (mixed_rows(N, K, g, -8, 8) / K ** 0.5).bfloat16()
    return w, w.double()


def operands_bf16(case):
    """CPU operands of one CASES_BF16 entry: activation rows spanning 2^-6 .. 2^6, weight rows spanning 2^-8 .. 2^8 over sqrt(K) (a row
    read in place of its neighbour is off by orders of magnitude), randn bias and residual, alpha = 1 + 0.1 randn.  The weight depends
    on (N, K) only and is shared by the cases of a table row."""
    B, N, K, mode, res, bias, gate = case
    w, w64 = _weight_bf16(N, K)
    g = torch.Generator().manual_seed(B * 1000 + N + K + mode + 17 * gate)
    x = mixed_rows(B, 2 * K if mode == 2 else K, g, -6, 6)
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    No = N // 2 if gate else N
    return dict(x=x, w=w, w64=w64, alpha=alpha if mode == 1 else None, bias=torch.randn(N, generator=g) if bias else None,
                res=torch.randn(B, No, generator=g) if res else None)


def reference_bf16(case, o, w64=None, bias=None):
    """(y64, bound): |y - y64| <= (c_gemv(K) + C_PROLOGUE[mode != 0]) * 2^-24 * (sum_k |w_k P(x)_k| + |bias| + |res|) per element, y64
    in fp64 on the bf16 weights; gate_out: the same bound on u and v carried through silu(u) * v (gate_carry).  `w64` / `bias`
    replace the case's own (the emulated defects)."""
    B, N, K, mode, res, _, gate = case
    w64 = o["w64"] if w64 is None else w64
    bias = o["bias"] if bias is None else bias
    x = o["x"]
    P = p_ref(x.double(), K, mode, o["alpha"].double() if mode == 1 else None)
    b64 = bias.double() if bias is not None else torch.zeros(N, dtype=torch.float64)
    h = P @ w64.t() + b64
    c = (c_gemv(K) + (Q.C_PROLOGUE if mode else 0)) * U
    dh = c * (P.abs() @ w64.abs().t() + b64.abs())
    if mode == 2:       # the fp32 silu(u) = u / (1 + expf(-u)) is -0 where expf(-u) overflows (u < -88.7): there |silu(u)| < 2^-121
        dh = dh + (x[:, K:].double().abs() * 2.0 ** -120) @ w64.abs().t()
    if gate:
        return gate_carry(h, dh)
    if res:
        return h + o["res"].double(), dh + c * o["res"].double().abs()
    return h, dh


# ---- fp32 weights: ops.linear at M <= 4 -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _weight_f32(N, K):
    g = torch.Generator().manual_seed(11 * N + K)
    w = mixed_rows(N, K, g, -8, 8) / K ** 0.5
    return w, w.double()


def operands_f32(case):
    """CPU operands of one CASES_F32 entry; as operands_bf16, gamma = 1 + 0.2 randn, beta = 0.1 randn, LayerScale 0.25 rand.  With
    `special rows` the first rows are, as far as M allows: 1000 + randn (far from zero mean: a one-pass variance loses it), a constant
    row (x_hat = 0: the output is beta @ w.T through the epilogue) and a row of magnitude 2^-20 (the variance far below eps)."""
    M, K, N, ln, bias, gelu, res, scale, special = case
    w, w64 = _weight_f32(N, K)
    g = torch.Generator().manual_seed(M * 1000 + N + K + 2 * ln + bias + 4 * gelu)
    x = mixed_rows(M, K, g, -6, 6)
    if special:
        # the far row comes from a generator of its own, so every case of one K sees the same row and the CPU test's verdict on the
        # one-pass variance does not hang on one case's luck: the fp32 difference E[x^2] - E[x]^2 is a multiple of 2^-4 here (the ulp of
        # 10^6) and can land near the true variance by chance (K = 512: 1.0625 against 0.9775)
        far = 1000 + torch.randn(K, generator=torch.Generator().manual_seed(1000))
        rows = [far, torch.full((K,), 0.7), 2.0 ** -20 * torch.randn(K, generator=g)]
        for i in range(min(M, 3)):
            x[i] = rows[i]
    return dict(x=x, w=w, w64=w64, gamma=1 + 0.2 * torch.randn(K, generator=g) if ln else None,
                beta=0.1 * torch.randn(K, generator=g) if ln else None, bias=torch.randn(N, generator=g) if bias else None,
                res=torch.randn(M, N, generator=g) if res else None, scale=0.25 * torch.rand(N, generator=g) if scale else None)


def reference_f32(case, o, w64=None):
    """(y64, bound) of ops.linear's GEMV route: |y - y64| <= 2^-24 * (c_gemv(K) * M + c_hat * M_hat + c_mean * M_mean), M the magnitude
    codec_streams.epilogue64 returns for sum_k |w_k a_k| (bias -> GELU -> res + scale * .), M_hat the same for the LayerNorm's
    magnitude codec_streams.layernorm64 returns and M_mean for the mean term rstd |gamma| mean|x| (the one tests/test_codec_streams_gpu.py
    _replay_linear adds), (c_hat, c_mean) = c_ln(K).  epilogue64 is linear in the magnitude it is given, so all three go through it in
    one call."""
    M, K, N, ln, bias, gelu, res, scale, _ = case
    w64 = o["w64"] if w64 is None else w64
    x64 = o["x"].double()
    d = lambda t: t.double() if t is not None else None
    if ln:
        eps = float(np.float32(EPS_LN))
        a, amag = CS.layernorm64(x64, o["gamma"], o["beta"], eps)
        rstd = 1 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + eps)
        mean_term = rstd * o["gamma"].double().abs() * x64.abs().mean(-1, keepdim=True)
        c_hat, c_mean = c_ln(K)
        mag = (a.abs() + (c_hat * amag + c_mean * mean_term) / c_gemv(K)) @ w64.abs().t()
    else:
        a = x64
        mag = a.abs() @ w64.abs().t()
    ref, m = CS.epilogue64(a @ w64.t(), mag, d(o["bias"]), d(o["res"]), d(o["scale"]), ACT_GELU if gelu else 0)
    return ref, c_gemv(K) * U * m
