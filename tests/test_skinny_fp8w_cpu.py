"""CPU checks of the weight-only fp8 skinny GEMM: the host restatement of its packed weight (tests/helpers/skinny_fp8w.py), the facts
its error bound rests on (exact decode, exact scale), the bound itself, and the three C-ABI entries in header, ctypes table and library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from rstnet_amd import _lib
from tests.helpers import lm_fp8w as Q
from tests.helpers import lm_operands as O
from tests.helpers import skinny_fp8w as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,K,interleave", [(33, 64, False), (64, 96, False), (64, 96, True), (96, 32, True)])
def test_packed_index_is_a_bijection(N, K, interleave):
    off = S.packed_offsets(N, K)
    n32 = S.rows32(N)
    assert off.shape == (n32, K)
    assert np.array_equal(np.sort(off.ravel()), np.arange(n32 * K)), "every byte of [ceil(N/32)*32, K] is written exactly once"
    # a lane's 16 bytes: 8 consecutive k of step 2p, then the same octet of step 2p + 1; a wave-level load is 1 KB contiguous
    for r, k in [(0, 0), (n32 - 1, K - 32), (17, 8)]:
        base = off[r, k]
        assert base % 16 == 0
        assert np.array_equal(off[r, k:k + 8], base + np.arange(8)) and np.array_equal(off[r, k + 16:k + 24], base + 8 + np.arange(8))
        assert base // 16 % 64 == 32 * ((k // 8) % 2) + r % 32
    src = S.src_rows(N, interleave)
    live = src[src >= 0]
    assert np.array_equal(np.sort(live), np.arange(N)), "every source row lands in exactly one packed row"


@pytest.mark.parametrize("N,K", [(64, 64), (160, 32)])
def test_interleaved_tiles_hold_matching_u_and_v_rows(N, K):
    g = torch.Generator().manual_seed(N + K)
    q = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.exp2(torch.randint(-20, 20, (N,), generator=g).double()).float()
    qp, sp = S.pack_weight_ref(q, s, interleave=True)
    dec = O.decode_fp8(qp, K)
    for t in range(N // 32):
        assert torch.equal(dec[32 * t:32 * t + 16], q[16 * t:16 * t + 16]), f"tile {t}: u rows 16t .. 16t+15"
        assert torch.equal(dec[32 * t + 16:32 * t + 32], q[N // 2 + 16 * t:N // 2 + 16 * t + 16]), f"tile {t}: the matching v rows"
        assert torch.equal(sp[32 * t:32 * t + 16], s[16 * t:16 * t + 16]) and torch.equal(sp[32 * t + 16:32 * t + 32], s[N // 2 + 16 * t:N // 2 + 16 * t + 16])


def test_plain_packing_pads_with_zero_bytes_and_zero_scales():
    N, K = 33, 64
    g = torch.Generator().manual_seed(1)
    q = torch.randint(1, 256, (N, K), generator=g, dtype=torch.int32).to(torch.uint8)
    s = torch.full((N,), 0.25)
    qp, sp = S.pack_weight_ref(q, s)
    dec = O.decode_fp8(qp, K)
    assert torch.equal(dec[:N], q) and not dec[N:].any() and torch.equal(sp[:N], s) and not sp[N:].any()


def test_decode_to_bf16_is_exact_for_every_finite_code():
    """The kernel keeps the upper 16 bits of the fp32 that v_cvt_pk_f32_fp8 yields: every finite e4m3fn value (4 significant bits,
    exponents 2^-9 .. 2^8) has a zero lower half, so the truncation drops nothing."""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    codes = codes[(codes & 0x7F) != 0x7F]
    v = codes.view(torch.float8_e4m3fn).float()
    assert len(v) == 254 and torch.isfinite(v).all()
    assert not (v.view(torch.int32) & 0xFFFF).any()
    assert torch.equal(v.bfloat16().float(), v)


def test_the_bound_is_the_bf16_packed_routes():
    """SPLIT_BOUND + _acc(K) (+ C_PROLOGUE * 2^-24 with a prologue), the constants of tests/test_lm_operands_gpu.py."""
    assert O.SPLIT_BOUND == 2.0 ** -16 and S.C_PROLOGUE == 32 and S.U == 2.0 ** -24
    for K in (288, 512, 1024, 4096, 8192):
        assert S.acc(K) == (K / 64 + 32) * 2.0 ** -24
        assert S.bound(K, 0) == 2.0 ** -16 + S.acc(K)
        assert S.bound(K, 1) == S.bound(K, 2) == 2.0 ** -16 + S.acc(K) + 32 * 2.0 ** -24
    # the absolute floor for subnormal outputs: half a unit of 2^-149 per wave and split, nothing next to a normal result
    assert S.underflow_floor(1) == 8 * 2.0 ** -150 and S.underflow_floor(16) == 2.0 ** -143 < 2.0 ** -23 * 2.0 ** -110


def test_scale_on_the_accumulator_equals_the_product_with_dequantised_weights():
    """fp32 emulation of one wave's chain: sum_k (hi + lo)_k q_k accumulated in fp32, then times 2^e, against the same chain on the
    dequantised weights q_k 2^e: equal bit for bit (a power of two commutes with every fp32 rounding while nothing leaves the normal
    range), and within the stated bound of the fp64 product."""
    g = torch.Generator().manual_seed(7)
    K = 512
    w = (torch.randn(4, K, generator=g) * torch.exp2(torch.tensor([-8.0, 0.0, 5.0, 9.0]))[:, None]).bfloat16()
    q, s = Q.quant_rows_ref(w)
    assert len(set(s.tolist())) == 4
    wq = Q.fp8_value(q).float().numpy()
    wd = Q.dequant_ref(q, s).float().numpy()
    x = torch.randn(K, generator=g).numpy()
    hi, lo = O.split_hi_lo(x)
    parts = (O.bf16_to_f32(hi), O.bf16_to_f32(lo))
    for n in range(4):
        a = b = np.float32(0)
        for k in range(K):
            for p in parts:
                a = np.float32(a + np.float32(p[k] * wq[n, k]))         # (4 x 8 significant bits: the product is exact in fp32)
                b = np.float32(b + np.float32(p[k] * wd[n, k]))
        assert np.float32(a * s[n].numpy()) == b
        ref = float(np.dot(x.astype(np.float64), wd[n].astype(np.float64)))
        mag = float(np.dot(np.abs(x).astype(np.float64), np.abs(wd[n]).astype(np.float64)))
        # (this chain is 2K long, 8 times the K/8 per wave of the kernel: scale the accumulation term accordingly)
        assert abs(float(b) - ref) <= (O.SPLIT_BOUND + 2 * K * S.U) * mag


def _header():
    text = open(os.path.join(ROOT, "include", "rstnet_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name,n_args", [("rst_skinny_pack_weight_fp8w", 8), ("rst_gemm_skinny_fp8w_supported", 3),
                                         ("rst_gemm_skinny_fp8w_f32", 15)])
def test_abi_entries(name, n_args):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    assert m, f"{name} is not declared in include/rstnet_hip.h"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args
    assert len(_lib.SIGNATURES[name]) == n_args
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name)
    lib.rst_version.restype = ctypes.c_int
    assert lib.rst_version() >= 124


def test_supported_predicate():
    lib = _lib.lib()
    ok = lambda B, N, K: bool(lib.rst_gemm_skinny_fp8w_supported(B, N, K))
    assert ok(3, 1001, 1024) and ok(1, 5, 32) and ok(64, 4096, 8192) and ok(32, 22528, 4096) and ok(33, 4096, 11264) and ok(8, 50, 704)
    assert not ok(8, 64, 272) and not ok(8, 64, 16) and not ok(65, 64, 1024) and not ok(0, 64, 1024) and not ok(8, 0, 1024)
