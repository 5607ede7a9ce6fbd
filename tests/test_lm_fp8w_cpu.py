"""CPU checks of the weight-only fp8 storage of the small-batch LM step: the host restatement of the quantiser
(tests/helpers/lm_fp8w.py) on hand-picked rows, its properties on random rows, and the two C-ABI entries in header, ctypes table
and library."""
import ctypes
import os
import re

import pytest
import torch

from rstnet_amd import _lib
from tests.helpers import lm_fp8w as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_picked_rows():
    """Exponents and bytes written down by hand: the all-zero row, amax = 448 * 2^e exactly and one ulp above, round-to-nearest-even
    ties in both directions, e4m3 subnormals, values below half the smallest subnormal, +-0, bf16-subnormal rows."""
    w, exps, want = Q.special_rows()
    q, s = Q.quant_rows_ref(w)
    assert torch.equal(s.double(), torch.exp2(exps.double())), (s, exps)
    for r, codes in want.items():
        assert q[r, :len(codes)].tolist() == codes, (r, [hex(c) for c in q[r, :len(codes)].tolist()])
    assert not q[0].any()
    # the smallest exponent: one less would push amax / 2^e above 448
    amax = w.double().abs().amax(dim=1)
    nz = amax > 0
    assert (amax[nz] / torch.exp2(exps.double()[nz]) <= 448).all() and (amax[nz] / torch.exp2(exps.double()[nz] - 1) > 448).all()


@pytest.mark.parametrize("spread", [0, 30])
def test_properties(spread):
    """|q| <= 448, no NaN code, q * 2^e exactly a bf16 number, and dequantise -> quantise -> dequantise is the identity."""
    g = torch.Generator().manual_seed(11 + spread)
    w = torch.randn(512, 4096, generator=g) * 0.02
    if spread:
        w = w * torch.exp2(torch.randint(-spread, spread + 1, (512, 1), generator=g).double()).float()
    w = w.bfloat16()
    w[3] = 0
    w[5, 17] = 448 * 2.0 ** -9
    w[5] = w[5].clamp(-448 * 2.0 ** -9, 448 * 2.0 ** -9)
    sp, _, _ = Q.special_rows(4096)
    w[8:8 + sp.shape[0]] = sp.bfloat16()
    q, s = Q.quant_rows_ref(w)
    assert ((q & 0x7F) <= 0x7E).all(), "0x7F / 0xFF are e4m3fn's NaN codes"
    assert s[3] == 1 and not q[3].any() and s[5] == 2.0 ** -9
    d = Q.dequant_ref(q, s)
    assert Q.is_exactly_bf16(d)
    q2, s2 = Q.quant_rows_ref(d)
    # (the exponent itself may drop by one -- an amax that rounds down to 224 * 2^e is 448 * 2^(e-1) -- the VALUES may not change)
    assert ((s2 == s) | (s2 == s / 2) | (d.abs().amax(dim=1) == 0)).all()
    assert torch.equal(Q.dequant_ref(q2, s2), d)
    # rms relative weight error of Gaussian rows (documented: 2.7 %)
    if not spread:
        rows = torch.arange(512) >= 64
        err = ((d[rows] - w[rows].double()).pow(2).sum() / w[rows].double().pow(2).sum()).sqrt().item()
        print(f"rms relative weight error {err:.4f}")
        assert 0.01 < err < 0.04


def _header():
    text = open(os.path.join(ROOT, "include", "rstnet_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name,n_args", [("rst_quant_rows_fp8", 6), ("rst_gemv_fp8w_supported", 3), ("rst_gemv_fp8w_f32", 16)])
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
    assert lib.rst_version() >= 122


def test_supported_predicate():
    lib = _lib.lib()
    ok = lambda B, N, K: bool(lib.rst_gemv_fp8w_supported(B, N, K))
    assert ok(1, 12288, 4096) and ok(2, 4096, 11264) and ok(1, 5, 16) and ok(4, 37, 2816) and ok(2, 50, 704)
    assert not ok(1, 64, 8) and not ok(1, 64, 4104) and not ok(5, 64, 1024) and not ok(0, 64, 1024)
    assert not ok(4, 64, 11264)           # 4 * 11264 fp32 do not fit the activation stage
