"""The reduced-precision operands of the LM's skinny GEMMs (csrc/lm_skinny.hip, lm_common.h, lm_attn.hip, lm_temporal.hip) read back and
held to stated bounds, element by element:

A  packed bf16 weights decode to w bit for bit (both layouts), pad rows zero;
B  packed activations: the identity prologue is exactly the emulated hi / lo split (tests/helpers/lm_operands.py), the RMSNorm / SiLU
   prologues are within the split bound plus their own fp32 error of an fp64 reference, pad rows zero;
C  the producers that write the packed operand themselves (the gated epilogue of the three GEMM routes, the attention's packed output);
D  the fp8 quantisers bit for bit against torch.float8_e4m3fn (scales and bytes);
E  the bf16 KV rings hold the round-to-nearest-even image of what the fp32 rings hold;
F  the products, on operands whose rows span 2^-20 .. 2^20 (activations) and 2^-30 .. 2^30 (weights), under a per-element bound
   relative to sum_k |x_k| |w_k| (the metric of tests/test_gemm_b3_gpu.py), so that one bad row of a tile cannot hide behind the
   tensor's largest element.

The device keeps fp32 denormals (gradual underflow): subnormal inputs and residuals are split exactly like the emulation does."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rstnet_amd import _lib, ops
from tests.helpers import lm_operands as O
from tests.helpers.gemv_bounds import mixed_rows as _mixed_rows, p_ref as _p_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SENTINEL = 0x5A5A               # bf16 pattern pre-filled where a kernel must not write (or must overwrite)
EPS = 1e-8

# fp32 error of the activation prologues, relative to |P(x)|, in units of 2^-24.  RMSNorm: sum of squares of positive terms over a
# chain of at most K/1024 fma + 6 wave-butterfly + 3 cross-wave additions (<= 20 roundings for K <= 11264), then / K, + eps, sqrt,
# reciprocal (1 each): 1/rms within 0.5 * 22 + 3 = 14; alpha * scale and x * that: 2 more -> 16.  SiLU gate: expf (<= 2), 1 + e, the
# division, the product with v: <= 6.  Both held to 32.
C_PROLOGUE = 32


def _acc(K: int) -> float:
    """fp32 accumulation bound of one output (relative to sum_k |x_k| |w_k|), every route: a lane's or a wave's sequential chain covers
    at most K/64 of the contraction (GEMV: 8 fma per 512-wide chunk per lane; skinny MFMA GEMM: K/8 per wave in 16-k steps, hi and lo
    each one accumulation -> K/64; fp8: K/128), plus at most 32 roundings for the MFMA's own 16-term sums, the lane / wave / split
    reductions, the per-row scales and the bias -- products themselves are exact (bf16 x bf16, e4m3 x e4m3, and fma for fp32 x bf16)."""
    return (K / 64 + 32) * U


# The fp8 matrix instruction (v_mfma_f32_32x32x16_fp8_fp8) does NOT sum its exact e4m3 products like a chain of fp32 additions: measured
# once on the MI355X, the backward error of the fp8 GEMM against its own quantised operands reaches 250 * 2^-24 ~ 2^-16 at K = 128
# (2.1M outputs; 9 * 2^-24 at K = 16384), where fp32 accumulation allows (K/64 + 32) * 2^-24 = 34.  The bf16 instruction stays within
# its fp32 bound (tests below).  Bound of the fp8 route: the instruction's own 2^-16, doubled, plus the fp32 accumulation bound.
FP8_MFMA_SUM = 2.0 ** -15


def _b32(B):
    return (B + 31) // 32 * 32


def _stream():
    return ops._stream()


def _p(t):
    return ops._ptr(t)


def _sentinel(*shape, dtype=torch.bfloat16):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV).view(dtype)


def _planes(xp, K):
    """packed [2, rows32, K] (or two flat planes) -> (hi, lo) uint16 [rows32, K]."""
    t = xp.view(torch.int16).reshape(2, -1)
    return O.bits16(O.decode_packed(t[0].cpu(), K)), O.bits16(O.decode_packed(t[1].cpu(), K))


def _value(hi, lo):
    return O.bf16_to_f32(hi).astype(np.float64) + O.bf16_to_f32(lo).astype(np.float64)


# hand-picked fp32 patterns planted into activation rows (see tests/test_lm_operands_cpu.py for what each one exercises)
SPECIALS = [0x3F80FFFF, 0x3F808080, 0xBF808080, 0x3F800101, 0x00000000, 0x80000000, 0x0000FFFF, 0x80012345,
            0x00812345, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x00800000, 0x007FFFFF]


def _plant(x: torch.Tensor):
    s = torch.from_numpy(np.array(SPECIALS, np.uint32).view(np.int32)).view(torch.float32)
    n = min(len(SPECIALS), x.shape[1])
    x[0, :n] = s[:n]
    x[-1, x.shape[1] - n:] = s[:n]


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 272, 4096])
@pytest.mark.parametrize("N", [1, 31, 33, 96, 4864])
def test_pack_weight_bf16_decodes_to_w(N, K):
    g = torch.Generator().manual_seed(N * 7 + K)
    w = torch.randint(-32768, 32768, (N, K), generator=g, dtype=torch.int32).to(torch.int16)    # every bit pattern is copied
    wd = w.to(DEV).view(torch.bfloat16)
    for inter in ((0, 1) if N % 32 == 0 else (0,)):
        wp = _sentinel(_b32(N), K)
        _lib.check(_lib.lib().rst_skinny_pack_weight_bf16(_p(wd), _p(wp), N, K, inter, _stream()))
        dec = O.decode_packed(wp.view(torch.int16).cpu(), K)
        if inter:       # tile t = rows 16t .. 16t+15 of W_u, then the same rows of W_v
            r = torch.arange(N)
            src = torch.where(r % 32 < 16, 0, N // 2) + (r // 32) * 16 + r % 16
            assert torch.equal(dec, w[src])
        else:
            assert torch.equal(dec[:N], w)
            assert not dec[N:].any(), "pad rows of the last weight tile must be zero"


# ---- B ------------------------------------------------------------------------------------------------------------------------
def _pack_act(x, B, K, mode, alpha=None, eps=EPS):
    xp = _sentinel(2, _b32(B), K)
    _lib.check(_lib.lib().rst_skinny_pack_act_f32(_p(x), _p(alpha), _p(xp), B, K, x.shape[1], mode, eps, _stream()))
    return _planes(xp, K)


@pytest.mark.parametrize("K", [16, 272, 4096, 11264])
@pytest.mark.parametrize("B", [3, 31, 32, 33, 64])
def test_pack_act_identity_is_the_exact_split(B, K):
    g = torch.Generator().manual_seed(B * 131 + K)
    x = _mixed_rows(B, K, g)
    _plant(x)
    hi, lo = _pack_act(x.to(DEV), B, K, 0)
    ehi, elo = O.split_hi_lo(x.numpy())
    bad = np.argwhere(~((hi[:B] == ehi) & O.same_bits16(lo[:B], elo)))
    assert bad.size == 0, [(int(b), int(k), hex(int(O.f32_bits(x[b, k].numpy()))), hex(int(hi[b, k])), hex(int(lo[b, k])))
                           for b, k in bad[:8]]
    assert not hi[B:].any() and not lo[B:].any(), "rows B .. ceil(B/32)*32 must be zero in both planes"


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("B,K", [(3, 4096), (33, 11264), (64, 272), (32, 16)])
def test_pack_act_prologues_within_the_split_bound(B, K, mode):
    """|P_ref - (hi + lo)| <= (2^-16 + C_PROLOGUE * 2^-24) |P_ref| per element, against P in fp64; rows scaled down to 2^-20, where
    the RMSNorm's eps (1e-8) dominates mean(x^2) ~ 2^-40."""
    g = torch.Generator().manual_seed(B * 17 + K + mode)
    x = _mixed_rows(B, 2 * K if mode == 2 else K, g)
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    hi, lo = _pack_act(x.to(DEV), B, K, mode, alpha.to(DEV) if mode == 1 else None)
    ref = _p_ref(x.double(), K, mode, alpha.double()).numpy()
    err = np.abs(_value(hi[:B], lo[:B]) - ref)
    bound = (O.SPLIT_BOUND + C_PROLOGUE * U) * np.abs(ref) + O.BF16_SUBNORMAL_HALF
    if mode == 2:       # the fp32 silu(u) = u / (1 + expf(-u)) is -0 where expf(-u) overflows (u < -88.7): there |silu(u)| < 2^-121
        bound = bound + np.abs(x[:, K:].double().numpy()) * 2.0 ** -120
    print(f"B={B} K={K} mode={mode}: max err / bound = {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    assert not hi[B:].any() and not lo[B:].any()


# ---- C ------------------------------------------------------------------------------------------------------------------------
def _silu_d(u):        # d/du silu(u) = s (1 + u (1 - s)), |.| < 1.1
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


def _gated_ref(P64, w64, b64, I, eps_h):
    """g = silu(u) * v of h = P w^T + b = [u | v] in fp64, and the bound on |g_fp32 - g| that an error of at most eps_h * (|P| |w|^T + |b|)
    in h carries (first order in the derivative, plus the product term), plus the fp32 silu / product (8 ulps) and the fp32 silu's flush
    to zero where expf(-u) overflows (|silu(u)| < 2^-119 there)."""
    h = P64 @ w64.t() + b64
    dh = eps_h * (P64.abs() @ w64.abs().t() + b64.abs())
    u, v, du, dv = h[:, :I], h[:, I:], dh[:, :I], dh[:, I:]
    gg = F.silu(u) * v
    dg = 1.1 * (v.abs() + dv) * du + F.silu(u).abs() * dv + 8 * U * gg.abs() + v.abs() * 2.0 ** -110
    return gg, dg


@pytest.mark.parametrize("route,B,I,K", [("packed", 5, 48, 512), ("packed", 33, 1408, 2816), ("x32", 3, 16, 256), ("x32", 40, 1024, 1024),
                                         ("split", 7, 256, 8192), ("split", 33, 1408, 4096)])
def test_gate_out_operand(route, B, I, K):
    """The gated epilogue of rst_gemm_skinny_bf16_f32 / rst_gemm_skinny_x32_bf16_f32 writes silu(u) * v as the packed operand
    [2][ceil(B/32)*32][I] of the next GEMM, zeros in the pad rows (the sentinel there is overwritten)."""
    g = torch.Generator().manual_seed(B + I + K)
    N = 2 * I
    x = _mixed_rows(B, K, g)
    w = (_mixed_rows(N, K, g, -8, 8) / K ** 0.5).bfloat16()
    bias = torch.randn(N, generator=g)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    wp = ops.skinny_pack_weight(wd, interleave_halves=True)
    gp = _sentinel(2, _b32(B), I)
    split = int(_lib.lib().rst_skinny_bf16_split_plan(B, N, K))
    assert (split > 1) == (route == "split")
    if route == "x32":
        _lib.check(_lib.lib().rst_gemm_skinny_x32_bf16_f32(_p(xd), None, 0.0, 0, K, _p(wp), None, _p(bd), None, B, N, K, N, _p(gp),
                                                           _stream()))
    else:
        xp = ops.skinny_pack_act(xd)
        ws = torch.empty(split, _b32(B), N, device=DEV) if split > 1 else None
        cnt = torch.zeros((N + 31) // 32, device=DEV, dtype=torch.int32) if split > 1 else None
        _lib.check(_lib.lib().rst_gemm_skinny_bf16_f32(_p(xp), _p(wp), None, _p(bd), None, B, N, K, N, _p(gp), split, _p(ws), _p(cnt),
                                                       _stream()))
    hi, lo = _planes(gp, I)
    gg, dg = _gated_ref(x.double(), w.double(), bias.double(), I, O.SPLIT_BOUND + _acc(K))
    gg, dg = gg.numpy(), dg.numpy()
    err = np.abs(_value(hi[:B], lo[:B]) - gg)
    bound = O.SPLIT_BOUND * (np.abs(gg) + dg) + dg + O.BF16_SUBNORMAL_HALF
    print(f"{route} B={B} I={I} K={K}: max err / bound = {np.max(err / bound):.3g}")
    assert (err <= bound).all()
    assert not hi[B:].any() and not lo[B:].any(), "the gated epilogue writes zeros into the pad rows of the batch tile"


@pytest.mark.parametrize("B", [3, 33])
@pytest.mark.parametrize("D", [64, 128])
def test_attention_packed_output(D, B):
    """rst_lm_attn_decode_f32(out_packed): the packed operand is exactly the hi / lo split of the fp32 form's result (same ring, same
    launch shape), within the split bound plus the attention's own fp32 error of an fp64 reference, and rows past B are untouched."""
    H, cap = 4, 300
    g = torch.Generator().manual_seed(D + B)
    vscale = torch.exp2(torch.randint(-20, 21, (B, 1, 1, 1), generator=g).double()).float()
    kc = torch.randn(B, H, cap, D, generator=g)
    vc = torch.randn(B, H, cap, D, generator=g) * vscale
    qkv = torch.randn(B, 3, H, D, generator=g)
    qkv[:, 2] *= vscale[:, :, :, 0]
    qkv = qkv.reshape(B, 3 * H * D)
    # the new step goes to slot cap - 2: slots 0 .. cap - 2 hold positions 0 .. cap - 2, all visible; the last slot is not yet written
    # (RingKVCache.complete maps it to no position)
    n = cap - 1
    pos = torch.full((1,), n - 1, dtype=torch.long, device=DEV)
    k1, v1, qd = kc.to(DEV), vc.to(DEV), qkv.to(DEV)
    out32 = ops.lm_attn_decode(qd, k1, v1, pos, rope=False, context=None)
    splits = ops.lm_attn_splits(cap, B * H)
    assert splits > 1
    k2, v2 = kc.to(DEV), vc.to(DEV)
    ws = torch.empty(B, H, splits, D + 2, device=DEV)
    cnt = torch.zeros(B, H, device=DEV, dtype=torch.int32)
    xp = _sentinel(2, _b32(B), H * D)
    _lib.check(_lib.lib().rst_lm_attn_decode_f32(_p(qd), _p(k2), _p(v2), _p(ws), _p(cnt), None, _p(pos), B, H, D, cap, 0, splits,
                                                3 * H * D, 0, ops.rope_coef(10000.0, D), H, 0, _p(xp), 0, None, _stream()))
    hi, lo = _planes(xp, H * D)
    o32 = out32.cpu().numpy()
    ehi, elo = O.split_hi_lo(o32)
    assert (hi[:B] == ehi).all() and (lo[:B] == elo).all()
    assert (hi[B:] == SENTINEL).all() and (lo[B:] == SENTINEL).all(), "rows past B must not be touched"
    # fp64 reference over the ring as the launch left it (the new key / value in the last slot)
    q = qkv.view(B, 3, H, D)[:, 0].double()
    keys, vals = k1[:, :, :n].cpu().double(), v1[:, :, :n].cpu().double()
    s = torch.einsum("bhd,bhcd->bhc", q, keys) / math.sqrt(D)
    p = torch.softmax(s, dim=-1)
    ref = torch.einsum("bhc,bhcd->bhd", p, vals).reshape(B, H * D).numpy()
    # scores: a D-term dot product in fp32 (<= D + 8 roundings) and the 1/sqrt(D) factor; exp(s - max) then carries twice the largest
    # score error (and 2 ulps of its own) into every weight and into their sum; the weighted sums over a head's slots add <= cap + 64
    ds = ((D + 8) * U * torch.einsum("bhd,bhcd->bhc", q.abs(), keys.abs()) / math.sqrt(D)).amax(dim=-1, keepdim=True)
    scale = torch.einsum("bhc,bhcd->bhd", p, vals.abs()).reshape(B, H * D)
    do = ((4 * ds + (2 * n + 64) * U).expand(B, H, 1).repeat_interleave(D, dim=2).reshape(B, H * D) * scale).numpy()
    err = np.abs(_value(hi[:B], lo[:B]) - ref)
    bound = O.SPLIT_BOUND * (np.abs(ref) + do) + do
    print(f"D={D} B={B}: max err / bound = {np.max(err / bound):.3g}")
    assert (err <= bound).all()


# ---- D ------------------------------------------------------------------------------------------------------------------------
FP8_TIES = [448.0, 1.0625, 1.1875, 3 * 2.0 ** -10, -1.0625, -1.1875, 2.0 ** -10, 0.0]   # scale 1; ties to even, subnormal ties


def _fp8_rows(rows, K, g, lo, hi):
    t = _mixed_rows(rows, K, g, lo, hi)
    t[0, :len(FP8_TIES)] = torch.tensor(FP8_TIES)
    t[0, len(FP8_TIES):] = t[0, len(FP8_TIES):].clamp(-400, 400)
    if rows > 2:
        t[1] = 0                                                  # an all-zero row: scale 1, zero bytes
    t[-1, -1] = 3.0 * t[-1].abs().max()                           # the row's max in its last element (the last 2048-chunk)
    return t


@pytest.mark.parametrize("N,K", [(1, 32), (33, 4096), (4864, 896), (40, 16384)])
def test_pack_weight_fp8_matches_torch(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = _fp8_rows(N, K, g, -30, 30).bfloat16()
    n32 = _b32(N)
    wp = torch.full((n32 * K,), 0xA5, dtype=torch.uint8, device=DEV)
    sc = torch.full((n32,), -1.0, device=DEV)
    wd = w.to(DEV)
    _lib.check(_lib.lib().rst_skinny_pack_weight_fp8(_p(wd), _p(wp), _p(sc), N, K, _stream()))
    q_ref, sc_ref = O.fp8_quant_ref(w.float())
    dec, sc = O.decode_fp8(wp.cpu(), K), sc.cpu()
    assert torch.equal(sc[:N].view(torch.int32), sc_ref.view(torch.int32))
    assert torch.equal(dec[:N], q_ref)
    assert (sc[N:] == 1).all() and not dec[N:].any()
    if N > 2:
        assert sc[1] == 1 and not dec[1].any()


def _pack_act_fp8(x, B, K, mode, alpha=None):
    b32 = _b32(B)
    xp = torch.full((b32 * K,), 0xA5, dtype=torch.uint8, device=DEV)
    xsc = torch.full((b32,), -1.0, device=DEV)
    _lib.check(_lib.lib().rst_skinny_pack_act_fp8(_p(x), _p(alpha), _p(xp), _p(xsc), B, K, x.shape[1], mode, EPS, _stream()))
    return O.decode_fp8(xp.cpu(), K), xsc.cpu()


@pytest.mark.parametrize("B,K", [(1, 2048), (3, 16384), (33, 4096), (64, 96)])
def test_pack_act_fp8_identity_matches_torch(B, K):
    g = torch.Generator().manual_seed(B * 5 + K)
    x = _fp8_rows(B, K, g, -20, 20)
    q, sc = _pack_act_fp8(x.to(DEV), B, K, 0)
    q_ref, sc_ref = O.fp8_quant_ref(x)
    assert torch.equal(sc[:B].view(torch.int32), sc_ref.view(torch.int32))
    assert torch.equal(q[:B], q_ref)
    assert (sc[B:] == 1).all() and not q[B:].any()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("B,K", [(3, 16384), (33, 4096), (64, 1024)])
def test_pack_act_fp8_prologues(B, K, mode):
    """RMSNorm / SiLU prologue in fp32 on the device, in fp64 here: >= 99.9 % of the bytes equal to the quantised fp64 result; every
    other byte one code away, and only where the exact value lies within 64 fp32 ulps of the rounding boundary between the two codes
    (the prologue's own error and the scale's, from an amax of the same few-ulp accuracy)."""
    g = torch.Generator().manual_seed(B * 3 + K + mode)
    x = _mixed_rows(B, 2 * K if mode == 2 else K, g)
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    qa, sc = _pack_act_fp8(x.to(DEV), B, K, mode, alpha.to(DEV) if mode == 1 else None)
    P = _p_ref(x.double(), K, mode, alpha.double())
    q_ref, sc_ref = O.fp8_quant_ref(P.float())
    assert ((sc[:B].double() / sc_ref.double() - 1).abs() <= 32 * U).all()
    q = qa[:B]
    diff = q != q_ref
    frac = diff.double().mean().item()
    print(f"B={B} K={K} mode={mode}: {int(diff.sum())} bytes of {q.numel()} differ ({frac:.2e})")
    assert frac <= 1e-3
    if diff.any():
        a, b = q[diff].int(), q_ref[diff].int()
        assert ((a & 0x80) == (b & 0x80)).all() and ((a & 0x7F) - (b & 0x7F)).abs().max() == 1
        t = (P / sc_ref.double()[:, None])[diff]
        mid = (O.fp8_to_f64(q[diff]) + O.fp8_to_f64(q_ref[diff])) / 2
        assert ((t - mid).abs() <= 64 * U * t.abs()).all()
    assert (sc[B:] == 1).all() and not qa[B:].any()


# ---- E ------------------------------------------------------------------------------------------------------------------------
def _rne_exceptions(ring16: torch.Tensor, ring32: torch.Tensor):
    """Elements of the bf16 ring that are not the RNE of the fp32 ring's: (count, count of them NOT within 2 fp32 ulps of a boundary)."""
    got = O.bits16(ring16)
    f = ring32.detach().cpu().contiguous().numpy()
    bad = ~O.same_bits16(got, O.bf16_rne(f))
    near = O.bf16_boundary_distance_ulps(f) <= 2
    return int(bad.sum()), int((bad & ~near).sum())


# values planted in v of the last step: ties to even (down / up), a tie carrying into the next binade, a tie rounding to +Inf, NaN,
# +-Inf, -0, a subnormal tie, one ulp either side of a tie
RING_SPECIALS = [0x3F808000, 0x3F818000, 0x3FFF8000, 0x7F7F8000, 0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00018000,
                 0x3F807FFF, 0x3F808001]


@pytest.mark.parametrize("D", [64, 128])
def test_bf16_ring_append_is_rne_of_the_fp32_ring(D):
    B, H, cap, steps = 2, 4, 300, 24
    g = torch.Generator().manual_seed(D)
    k32 = torch.zeros(B, H, cap, D, device=DEV)
    v32 = torch.zeros_like(k32)
    k16 = torch.zeros(B, H, cap, D, device=DEV, dtype=torch.bfloat16)
    v16 = torch.zeros_like(k16)
    p32 = torch.zeros(1, dtype=torch.long, device=DEV)
    p16 = torch.zeros(1, dtype=torch.long, device=DEV)
    vs = torch.from_numpy(np.array(RING_SPECIALS, np.uint32).view(np.int32)).view(torch.float32)
    for s in range(steps):
        qkv = _mixed_rows(B, 3 * H * D, g, -6, 6)
        if s == steps - 1:
            qkv[0, 2 * H * D:2 * H * D + len(vs)] = vs
        qkv = qkv.to(DEV)
        ops.lm_attn_decode(qkv, k32, v32, p32, rope=True, context=None)       # keys rotated in fp32 (angles up to `steps` rad)
        ops.lm_attn_decode(qkv, k16, v16, p16, rope=True, context=None)
        p32.add_(1)
        p16.add_(1)
    nk, far_k = _rne_exceptions(k16[:, :, :steps], k32[:, :, :steps])
    nv, far_v = _rne_exceptions(v16[:, :, :steps], v32[:, :, :steps])
    print(f"D={D}: keys off RNE of the fp32 ring: {nk} (beyond 2 ulps of a boundary: {far_k}); values: {nv}")
    assert far_k == 0 and nk <= 4 and nv == 0
    ring = O.bits16(v16[0, 0, steps - 1, :len(vs)])
    want = O.bf16_rne(vs.numpy())
    assert O.same_bits16(ring, want).all(), [hex(int(a)) for a in ring]
    assert torch.equal(v32[0, 0, steps - 1, :len(vs)].cpu().view(torch.int32), vs.view(torch.int32))    # fp32 ring: the bits, copied


def test_temporal_frame_bf16_ring_is_rne_of_the_fp32_ring():
    """rst_temporal_decode_frame, layer 0 (its k / v depend on the step's x only): bf16 ring = RNE of the fp32 ring's, up to elements
    within 2 fp32 ulps of a rounding boundary (the two launches are different kernel instances)."""
    from tests.test_temporal_frame_gpu import _run, _transformer
    g = torch.Generator(device=DEV).manual_seed(3)
    xs = [torch.randn(1, 4096, device=DEV, generator=g) for _ in range(12)]
    _, st32, kv32 = _run(_transformer(1, torch.float32), xs, True)
    _, st16, kv16 = _run(_transformer(1, torch.bfloat16), xs, True)
    assert st32 == [0, 0, 0, 0] and st16 == [0, 0, 0, 0]
    n = len(xs)
    for i, name in enumerate("kv"):
        cnt, far = _rne_exceptions(kv16[i][:, :, :n], kv32[i][:, :, :n])
        print(f"temporal frame layer 0 {name}: {cnt} elements off RNE (beyond 2 ulps of a boundary: {far})")
        assert far == 0 and cnt <= max(4, kv16[i][:, :, :n].numel() // 10000)


# ---- F ------------------------------------------------------------------------------------------------------------------------
def _operands(B, N, K, g, mode):
    x = _mixed_rows(B, 2 * K if mode == 2 else K, g)
    w = _mixed_rows(N, K, g, -30, 30).bfloat16()
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    return x, w, alpha


def _backward_error(y, P64, w64):
    ref = P64 @ w64.t()
    return float(((y.double().cpu() - ref).abs() / (P64.abs() @ w64.abs().t())).max())


# (B, N, K, prologue): every batch-tile count, ragged N (N % 32 and N % 4 != 0), K either side of the split thresholds (8192 up to 32
# rows, 4096 above), 1 .. 4 column tiles per workgroup (with a K split: 4 / 2; without: ceil(tiles / 256 CUs)), both operand routes
SKINNY = [(3, 1001, 1024, 0), (4, 33, 4096, 1), (5, 1001, 8192, 0), (31, 9001, 272, 2), (32, 17001, 512, 1), (32, 25001, 256, 0),
          (33, 1001, 2816, 0), (33, 4099, 4096, 1), (63, 17001, 1024, 0), (64, 4099, 8192, 2), (64, 9001, 272, 0), (31, 33, 16, 0)]


@pytest.mark.parametrize("B,N,K,mode", SKINNY)
def test_gemm_skinny_elementwise_bound(B, N, K, mode):
    g = torch.Generator().manual_seed(B * 1000 + N + K)
    x, w, alpha = _operands(B, N, K, g, mode)
    y = ops.gemm_skinny(x.to(DEV), w.to(DEV), prologue=mode, alpha=alpha.to(DEV) if mode == 1 else None, eps=EPS)
    x32 = mode in (0, 1) and K <= ops.SKINNY_X32_MAX_K and K % 256 == 0
    split = 1 if x32 else int(_lib.lib().rst_skinny_bf16_split_plan(B, N, K))
    e = _backward_error(y, _p_ref(x.double(), K, mode, alpha.double()), w.double())
    bound = O.SPLIT_BOUND + _acc(K) + (C_PROLOGUE * U if mode else 0)
    print(f"B={B} N={N} K={K} mode={mode} route={'x32' if x32 else 'packed'} split={split}: backward error {e / U:.1f} * 2^-24 "
          f"(bound {bound / U:.0f})")
    assert e <= bound


@pytest.mark.parametrize("B,I,K,bias", [(3, 1408, 512, True), (5, 96, 8192, True), (33, 2816, 4096, False), (64, 4864, 896, True)])
def test_gated_pair_elementwise_bound(B, I, K, bias):
    """res + W_out (silu(u) * v), [u | v] = W_in rmsnorm(x): the first GEMM's bound carried through the gate (as in test_gate_out_operand),
    then the second GEMM's split and accumulation bounds on top."""
    g = torch.Generator().manual_seed(B + I + K)
    x = _mixed_rows(B, K, g)
    w_in = (_mixed_rows(2 * I, K, g, -8, 8) / K ** 0.5).bfloat16()
    w_out = (_mixed_rows(K, I, g, -8, 8) / I ** 0.5).bfloat16()
    b_in = torch.randn(2 * I, generator=g) if bias else torch.zeros(2 * I)
    b_out = torch.randn(K, generator=g) if bias else torch.zeros(K)
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    dev = lambda t: t.to(DEV) if bias else None
    y = ops.lm_gated_pair(x.to(DEV), w_in.to(DEV), w_out.to(DEV), alpha=alpha.to(DEV), eps=EPS, res=x.to(DEV), bias_in=dev(b_in),
                          bias_out=dev(b_out))
    P = _p_ref(x.double(), K, 1, alpha.double())
    gg, dg = _gated_ref(P, w_in.double(), b_in.double(), I, O.SPLIT_BOUND + _acc(K) + C_PROLOGUE * U)
    wo = w_out.double()
    ref = x.double() + gg @ wo.t() + b_out.double()
    g_abs = gg.abs() + dg
    bound = (O.SPLIT_BOUND * g_abs + dg) @ wo.abs().t() + _acc(I) * (x.double().abs() + b_out.double().abs() + g_abs @ wo.abs().t())
    r = ((y.double().cpu() - ref).abs() / bound).max().item()
    print(f"B={B} I={I} K={K}: max err / bound = {r:.3g}")
    assert r <= 1


FP8 = [(3, 1001, 1024, 0), (5, 65, 16384, 0), (32, 4099, 4096, 1), (33, 1001, 2048, 2), (64, 17001, 512, 0), (32, 65537, 128, 0)]


@pytest.mark.parametrize("B,N,K,mode", FP8)
def test_gemm_skinny_fp8_elementwise_bound(B, N, K, mode):
    """Against the product of its own quantised operands (read back from the packing launches): e4m3 x e4m3 products are exact, so
    y = scale_x[b] scale_w[n] sum_k qx qw up to the instruction's summation (FP8_MFMA_SUM) and fp32 accumulation, relative to
    scale_x[b] scale_w[n] sum_k |qx| |qw|: a wrong scale on one row, or one row's bytes, is an error of order 1."""
    g = torch.Generator().manual_seed(B * 77 + N + K)
    x, w, alpha = _operands(B, N, K, g, mode)
    xd, wd, ad = x.to(DEV), w.to(DEV), alpha.to(DEV) if mode == 1 else None
    y = ops.gemm_skinny_fp8(xd, wd, prologue=mode, alpha=ad, eps=EPS)
    qx, sx = _pack_act_fp8(xd, B, K, mode, ad)
    wp, sw = ops.skinny_pack_weight_fp8(wd)
    qw = O.fp8_to_f64(O.decode_fp8(wp.cpu(), K)[:N])
    qx = O.fp8_to_f64(qx[:B])
    s = sx[:B].double()[:, None] * sw.cpu()[:N].double()[None, :]
    ref = s * (qx @ qw.t())
    e = float(((y.double().cpu() - ref).abs() / (s * (qx.abs() @ qw.abs().t())).clamp_min(1e-300)).max())
    print(f"fp8 B={B} N={N} K={K} mode={mode}: backward error {e / U:.1f} * 2^-24 (bound {(FP8_MFMA_SUM + _acc(K)) / U:.0f})")
    assert e <= FP8_MFMA_SUM + _acc(K)


@pytest.mark.parametrize("B,N,K,mode", [(1, 1001, 4096, 0), (2, 4099, 1024, 1), (1, 12288, 4096, 0), (2, 33, 11264, 2), (1, 31, 16, 0)])
def test_gemv_bf16_elementwise_bound(B, N, K, mode):
    """B <= 2: fp32 activations against bf16 weights in fma chains (no split): accumulation and prologue bounds only."""
    g = torch.Generator().manual_seed(B * 9 + N + K)
    x, w, alpha = _operands(B, N, K, g, mode)
    y = ops.gemv_bf16(x.to(DEV), w.to(DEV), prologue=mode, alpha=alpha.to(DEV) if mode == 1 else None, eps=EPS)
    e = _backward_error(y, _p_ref(x.double(), K, mode, alpha.double()), w.double())
    bound = _acc(K) + (C_PROLOGUE * U if mode else 0)
    print(f"gemv B={B} N={N} K={K} mode={mode}: backward error {e / U:.1f} * 2^-24 (bound {bound / U:.0f})")
    assert e <= bound
