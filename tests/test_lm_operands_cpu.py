"""The CPU restatements of tests/helpers/lm_operands.py on hand-picked bit patterns: the hi / lo split of the skinny GEMM's activations
(its 2^-16 bound, the carry into the next binade, ties, +-0, subnormals, +-Inf, NaN), bf16 round to nearest even, and the two
operand layouts (the decoding reshapes against the index formulas of lm_common.h / lm_skinny.hip).  The GPU side of the same
emulations is tests/test_lm_operands_gpu.py."""
import numpy as np
import torch

from tests.helpers import lm_operands as O


def _f(*bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_split_hi_lo_hand_picked_patterns():
    x = _f(0x3F800000,          # 1.0: hi exact, lo +0
           0x3F80FFFF,          # residual 2^-7 - 2^-23 rounds up into the next binade: lo = 2^-7
           0x3F808080,          # residual 2^-8 + 2^-16: a tie, rounded half-up (away from zero): the 2^-16 worst case
           0xBF808080,          # the same, negative: the magnitude rounds up
           0x3F800101,          # residual 2^-15 + 2^-23: a tie one binade lower
           0x00000000, 0x80000000,  # +-0
           0x0000FFFF,          # subnormal below bf16's top subnormals: hi = 0, lo rounds up to the smallest bf16 subnormal
           0x00812345,          # normal x with a subnormal residual
           0x7F7FFFFF,          # FLT_MAX: the residual 2^120 - 2^104 carries into lo = 2^120
           0x7F800000, 0xFF800000,  # +-Inf: hi = +-Inf, residual Inf - Inf = NaN
           0x7FC00000)          # NaN
    hi, lo = O.split_hi_lo(x)
    assert hi.tolist()[:5] == [0x3F80, 0x3F80, 0x3F80, 0xBF80, 0x3F80]
    assert lo.tolist()[:5] == [0x0000, 0x3C00, 0x3B81, 0xBB81, 0x3800 | 0x01]
    assert hi[5] == 0x0000 and lo[5] == 0x0000 and hi[6] == 0x8000 and lo[6] == 0x0000
    assert hi[7] == 0x0000 and lo[7] == 0x0001
    assert hi[8] == 0x0081 and lo[8] == ((0x2345 + 0x8000) >> 16)
    assert hi[9] == 0x7F7F and lo[9] == 0x7B80
    assert hi[10] == 0x7F80 and hi[11] == 0xFF80 and O.is_nan16(lo[10:]).all()
    assert O.is_nan16(hi[12])
    # hi + lo against x, and the stated bound where x is finite
    fin = np.isfinite(x)
    err = np.abs(x[fin].astype(np.float64) - O.bf16_to_f32(hi[fin]).astype(np.float64) - O.bf16_to_f32(lo[fin]).astype(np.float64))
    assert (err <= O.SPLIT_BOUND * np.abs(x[fin].astype(np.float64)) + O.BF16_SUBNORMAL_HALF).all()
    assert err[2] == 2.0 ** -16                                    # the bound is attained


def test_split_hi_lo_bound_over_a_wide_range():
    g = np.random.default_rng(0)
    x = (g.standard_normal(1 << 20) * np.exp2(g.integers(-100, 100, 1 << 20))).astype(np.float32)
    hi, lo = O.split_hi_lo(x)
    xd = x.astype(np.float64)
    err = np.abs(xd - O.bf16_to_f32(hi).astype(np.float64) - O.bf16_to_f32(lo).astype(np.float64))
    rel = err / np.abs(xd)
    assert rel.max() <= O.SPLIT_BOUND
    assert rel.max() > 0.9 * O.SPLIT_BOUND                         # and it is the tight one: 2^-17 (the old statement) is exceeded
    # hi is a truncation (never larger in magnitude than x), lo carries the sign of x
    assert (np.abs(O.bf16_to_f32(hi)) <= np.abs(x)).all()
    nz = O.bf16_to_f32(lo) != 0
    assert (np.sign(O.bf16_to_f32(lo)[nz]) == np.sign(x[nz])).all()


def test_bf16_rne_hand_picked_patterns():
    x = _f(0x3F808000,          # tie, even below: stays
           0x3F818000,          # tie, odd below: up
           0x3F807FFF, 0x3F808001,
           0x3FFF8000,          # tie whose round-up carries into the next binade: 2.0
           0x7F7F8000,          # tie at the top of the range: rounds to +Inf
           0x00008000, 0x00018000,  # subnormal ties
           0x80000000, 0x7F800000, 0xFF800000,
           0x7FC00001, 0xFF800001)  # NaNs (the second signalling): stay NaN, sign kept
    r = O.bf16_rne(x)
    assert r.tolist()[:11] == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x4000, 0x7F80, 0x0000, 0x0002, 0x8000, 0x7F80, 0xFF80]
    assert O.is_nan16(r[11:]).all() and r[11] >> 15 == 0 and r[12] >> 15 == 1
    # agrees with torch's conversion on every non-NaN pattern of a random sample
    u = np.random.default_rng(1).integers(0, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32)
    f = u.view(np.float32)
    ok = ~np.isnan(f)
    t = torch.from_numpy(f[ok].copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (O.bf16_rne(f[ok]) == t).all()
    assert O.bf16_boundary_distance_ulps(_f(0x3F808000, 0x3F807FFF, 0x3F800000)).tolist() == [0, 1, 0x8000]


def test_layout_decoders_match_the_index_formulas():
    for rows, K in ((32, 16), (64, 48), (96, 272)):
        n = rows * K
        code = torch.arange(n, dtype=torch.int32)
        r, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
        idx = O.packed_index(r, k, K)
        assert sorted(idx.ravel().tolist()) == list(range(n))     # a permutation of the plane
        assert np.array_equal(O.decode_packed(code, K).numpy(), idx)
    for rows, K in ((32, 32), (64, 96), (96, 320)):
        n = rows * K
        code = torch.arange(n, dtype=torch.int32)
        r, k = np.meshgrid(np.arange(rows), np.arange(K), indexing="ij")
        idx = O.fp8_packed_index(r, k, K)
        assert sorted(idx.ravel().tolist()) == list(range(n))
        assert np.array_equal(O.decode_fp8(code, K).numpy(), idx)


def test_fp8_reference_quantiser():
    t = torch.zeros(3, 64)
    t[0, 0] = 448.0                                               # scale exactly 1: the bytes are the e4m3 codes of the values
    t[0, 1:5] = torch.tensor([1.0625, 1.1875, 3 * 2.0 ** -10, -1.0625])   # ties: RNE -> 1.0, 1.25, 2^-8 (even subnormal code), -1.0
    t[2] = torch.linspace(-3, 3, 64)
    q, sc = O.fp8_quant_ref(t)
    assert sc[0] == 1.0 and sc[1] == 1.0 and sc[2] == np.float32(3.0) / np.float32(448.0)
    assert not q[1].any()
    assert O.fp8_to_f64(q[0, :5]).tolist() == [448.0, 1.0, 1.25, 2.0 ** -8, -1.0]
