"""CPU checks of the weight-only MXFP4 storage of the small-batch LM step: the host restatement of the quantiser
(tests/helpers/lm_mxfp4.py) on hand-picked blocks, its properties on random rows, the refusals, and the three C-ABI entries in
header, ctypes table and library."""
import ctypes
import os
import re

import pytest
import torch

from rstnet_amd import _lib
from tests.helpers import lm_mxfp4 as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_picked_blocks():
    """Exponents and codes written down by hand: the all-zero block, amax = 6 * 2^e exactly and one bf16 ulp above, every tie of the
    e2m1 grid in both signs, +-0, a negative amax, bf16-subnormal blocks at the clamp e = -125, amax just below 2^120."""
    w, exps, want = Q.special_blocks()
    q, s = Q.quant_blocks_ref(w)
    assert s.shape == (w.shape[0], 1) and torch.equal(s[:, 0].long() - 127, exps), (s[:, 0].long() - 127, exps)
    codes = Q.codes_of(q)
    for r, c in want.items():
        assert codes[r, :len(c)].tolist() == c, (r, [hex(v) for v in codes[r, :len(c)].tolist()])
        assert not codes[r, len(c):].any()
    assert not q[0].any()
    # the smallest exponent: one less would push amax / 2^e above 6 (where the clamp does not bind)
    amax = w.double().abs().amax(dim=1)
    e = exps.double()
    free = (amax > 0) & (exps > Q.E_MIN)
    assert (amax[free] / torch.exp2(e[free]) <= 6).all() and (amax[free] / torch.exp2(e[free] - 1) > 6).all()
    assert (amax / torch.exp2(e) <= 6).all()
    assert Q.is_exactly_bf16(Q.dequant_ref(q, s))


def _spread_rows(N, K, spread, g):
    w = torch.randn(N, K, generator=g) * 0.02
    if spread:
        w = (w.view(N, K // 32, 32) * torch.exp2(torch.randint(-spread, spread + 1, (N, K // 32, 1), generator=g).double()).float()).view(N, K)
    return w.bfloat16()


@pytest.mark.parametrize("spread", [0, 30])
def test_properties(spread):
    """codes <= 7 in magnitude, amax / 2^e <= 6 and > 6 at e - 1, code * 2^e exactly a finite bf16 number and normal or zero, and
    dequantise -> quantise -> dequantise is the identity on values."""
    g = torch.Generator().manual_seed(11 + spread)
    w = _spread_rows(256, 4096, spread, g)
    w[3] = 0
    w[5, :32] = w[5, :32].clamp(-6 * 2.0 ** -9, 6 * 2.0 ** -9)
    w[5, 17] = 6 * 2.0 ** -9
    sp, exps, _ = Q.special_blocks()
    sp, exps = sp[:-1], exps[:-1]          # (not the block below 2^120: its amax rounds UP to 2^120, which the second pass would refuse)
    w[8, :sp.numel()] = sp.flatten().bfloat16()
    q, s = Q.quant_blocks_ref(w)
    assert q.dtype == torch.uint8 and q.shape == (256, 2048) and s.dtype == torch.uint8 and s.shape == (256, 128)
    assert ((Q.codes_of(q) & 7) <= 7).all() and Q.codes_of(q).max() <= 15
    assert (s[3] == 127).all() and not q[3].any() and s[5, 0] == 127 - 9
    assert torch.equal(s[8, :sp.shape[0]].long() - 127, exps)
    e = s.double() - 127
    amax = w.double().view(256, 128, 32).abs().amax(dim=-1)
    assert (amax / torch.exp2(e) <= 6).all()
    free = (amax > 0) & (e > Q.E_MIN)
    assert (amax[free] / torch.exp2(e[free] - 1) > 6).all()
    d = Q.dequant_ref(q, s)
    assert Q.is_exactly_bf16(d)
    assert ((d == 0) | (d.abs() >= 2.0 ** -126)).all(), "code * 2^e must be a normal number"
    q2, s2 = Q.quant_blocks_ref(d)
    # (the exponent itself may drop when a block's amax rounds down, e.g. to 3 * 2^e = 6 * 2^(e-1) -- the VALUES may not change)
    assert (s2 <= s).all()
    assert torch.equal(Q.dequant_ref(q2, s2), d)
    # rms relative weight error of Gaussian rows (documented: 11.5 %)
    if not spread:
        rows = torch.arange(256) >= 16
        err = ((d[rows] - w[rows].double()).pow(2).sum() / w[rows].double().pow(2).sum()).sqrt().item()
        print(f"rms relative weight error {err:.4f}")
        assert 0.09 < err < 0.14


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan"), 2.0 ** 121, -2.0 ** 120])
def test_refusals(bad):
    w = torch.ones(4, 64, dtype=torch.bfloat16)
    w[2, 37] = bad
    with pytest.raises(ValueError):
        Q.quant_blocks_ref(w)
    with pytest.raises(ValueError):
        Q.quant_blocks_ref(torch.ones(4, 48, dtype=torch.bfloat16))
    Q.quant_blocks_ref(torch.full((1, 32), 1.9921875 * 2.0 ** 119, dtype=torch.bfloat16))


def _header():
    text = open(os.path.join(ROOT, "include", "rstnet_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name,n_args", [("rst_quant_blocks_mxfp4", 6), ("rst_gemv_mxfp4w_supported", 3), ("rst_gemv_mxfp4w_f32", 16)])
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
    assert lib.rst_version() >= 123


def test_supported_predicate():
    lib = _lib.lib()
    ok = lambda B, N, K: bool(lib.rst_gemv_mxfp4w_supported(B, N, K))
    assert ok(1, 12288, 4096) and ok(2, 4096, 11264) and ok(1, 5, 32) and ok(4, 37, 2816) and ok(2, 50, 704)
    assert not ok(1, 64, 16) and not ok(1, 64, 48) and not ok(1, 64, 4112) and not ok(5, 64, 1024) and not ok(0, 64, 1024)
    assert ok(4, 64, 8192) and not ok(4, 64, 8224)      # 4 * roundup(8224, 2048) fp32 do not fit the activation stage
    assert not ok(4, 64, 11264) and not ok(1, 64, 32800)
