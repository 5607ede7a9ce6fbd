"""The default GEMVs of csrc/lm_step.hip held to per-element bounds against fp64, at every instance rst_launch_gemv dispatches to:
ops.gemv_bf16 (bf16 weights: gemv_kernel<B, 2 | 4>, gemv_norm_kernel<gate>, gemv_ksplit_kernel) and ops.linear at M <= 4 (fp32 weights,
LayerNorm prologue, GELU / LayerScale / residual epilogue: gemv_kernel<B, 2, f32>).  Cases, operands, references and bounds come from
tests/helpers/gemv_bounds.py; tests/test_gemv_bounds_cpu.py checks there that the tables reach every instance, grid-strided and ragged,
and that the bounds separate plain fp32 arithmetic from a one-pass variance, a wrong bias half and a dropped tail chunk.

Activation rows span 2^-6 .. 2^6 and weight rows 2^-8 .. 2^8 over sqrt(K), so an output computed from a neighbouring row, a stale
residual or a partial sum left out is off by orders of magnitude more than the bound, which is relative to each element's own
sum_k |w_k P(x)_k| + |bias| + |res|."""
import functools

import pytest
import torch

from rstnet_amd import _lib, ops
from tests.helpers import gemv_bounds as GB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0


def _dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=1)
def _weight_on_device(kind, N, K):      # the cases of a table row share one weight: one upload
    return (GB._weight_bf16(N, K) if kind == "bf16" else GB._weight_f32(N, K))[0].to(DEV)


def _flags(**kw):
    return "".join(f" {k}" for k, v in kw.items() if v)


def _id_bf16(c):
    return f"B{c[0]}-{c[1]}x{c[2]}-p{c[3]}" + _flags(res=c[4], bias=c[5], gate=c[6]).replace(" ", "-")


def _id_f32(c):
    return f"M{c[0]}-{c[1]}to{c[2]}" + _flags(ln=c[3], bias=c[4], gelu=c[5], res=c[6], scale=c[7]).replace(" ", "-")


def _assert_within(y, ref, bound, what):
    err = (y - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err / bound = {ratio:.3g}")
    bad = (~(err <= bound)).nonzero()
    assert bad.numel() == 0, (what, f"{bad.shape[0]} elements outside the bound",
                              [(int(b), int(n), float(y[b, n]), float(ref[b, n]), float(bound[b, n])) for b, n in bad[:8]])


@pytest.mark.parametrize("case", GB.CASES_BF16, ids=_id_bf16)
def test_gemv_bf16_bound(case):
    """|y - y64| <= (c_gemv(K) + C_PROLOGUE[mode != 0]) * 2^-24 * (sum_k |w_k P(x)_k| + |bias| + |res|) per element, y64 in fp64 on
    the bf16 weights (helpers.gemv_bounds.reference_bf16; gate_out: the bound on u and v carried through silu(u) * v)."""
    B, N, K, mode, res, bias, gate = case
    r = GB.route_bf16(case)
    o = GB.operands_bf16(case)
    y = ops.gemv_bf16(_dev(o["x"]), _weight_on_device("bf16", N, K), prologue=mode, alpha=_dev(o["alpha"]), eps=GB.EPS_RMS, res=_dev(o["res"]),
                      bias=_dev(o["bias"]), gate_out=gate).cpu().double()
    assert y.shape == (B, N // 2 if gate else N)
    ref, bound = GB.reference_bf16(case, o)
    _assert_within(y, ref, bound, f"B={B} N={N} K={K} mode={mode}{_flags(res=res, bias=bias, gate=gate)} -> {r['name']} groups={r['groups']} "
                                  f"grid={r['grid']}{_flags(strided=r['strided'], ragged=r['ragged'])}")


@pytest.mark.parametrize("case", GB.CASES_F32, ids=_id_f32)
def test_gemv_f32_bound(case):
    """ops.linear at M <= 4: the GEMV route (no GEMM profile row), within c_gemv(K) of codec_streams.epilogue64's magnitude plus the
    LayerNorm prologue's own terms (helpers.gemv_bounds.reference_f32, c_ln)."""
    M, K, N, ln, bias, gelu, res, scale, special = case
    r = GB.route_f32(case)
    o = GB.operands_f32(case)
    ops.PROFILE = []
    try:
        y = ops.linear(_dev(o["x"]), _weight_on_device("f32", N, K), _dev(o["bias"]), res=_dev(o["res"]), scale=_dev(o["scale"]),
                       act_out=ops.ACT_GELU if gelu else ops.ACT_NONE, ln=(_dev(o["gamma"]), _dev(o["beta"]), GB.EPS_LN) if ln else None)
        torch.cuda.synchronize()
        rows = list(ops.PROFILE)
    finally:
        ops.PROFILE = None
    assert rows == [], f"ops.linear at M = {M} took a GEMM route: {[p[0] for p in rows]}"
    assert y.shape == (M, N)
    ref, bound = GB.reference_f32(case, o)
    _assert_within(y.cpu().double(), ref, bound, f"M={M} K={K} N={N}{_flags(ln=ln, bias=bias, gelu=gelu, res=res, scale=scale, rows=special)} "
                                                 f"-> {r['name']} groups={r['groups']} grid={r['grid']}{_flags(strided=r['strided'])}")


def test_all_zero_row_under_rmsnorm_gives_bias_plus_res():
    """x = 0: rsqrt(eps) is finite, every product is zero and the output is the one fp32 addition bias + res, bit for bit."""
    case = (2, 37, 1032, 1, True, True, False)
    o = GB.operands_bf16(case)
    o["x"][0] = 0
    y = ops.gemv_bf16(_dev(o["x"]), _dev(o["w"]), prologue=1, alpha=_dev(o["alpha"]), eps=GB.EPS_RMS, res=_dev(o["res"]), bias=_dev(o["bias"])).cpu()
    assert torch.isfinite(y).all()
    assert torch.equal(y[0], o["res"][0] + o["bias"])
    ref, bound = GB.reference_bf16(case, o)
    _assert_within(y.double(), ref, bound, "zero row + live row")


def test_second_call_overwrites_every_element_of_out():
    case = (3, 37, 1032, 0, True, True, False)
    o = GB.operands_bf16(case)
    args = dict(res=_dev(o["res"]), bias=_dev(o["bias"]))
    first = ops.gemv_bf16(_dev(o["x"]), _dev(o["w"]), **args)
    out = torch.full((3, 37), float("nan"), device=DEV)
    got = ops.gemv_bf16(_dev(o["x"]), _dev(o["w"]), out=out, **args)
    assert got is out and torch.equal(out.cpu(), first.cpu())
    gated = torch.full((3, 18), float("nan"), device=DEV)
    ops.gemv_bf16(_dev(o["x"]), _dev(o["w"][:36].contiguous()), bias=_dev(o["bias"][:36].contiguous()), out=gated, gate_out=True)
    assert not torch.isnan(gated).any()


def test_unsupported_arguments_are_refused():
    """Each raises before anything is launched: the sentinel-filled output is untouched."""
    def refused(call, out, what):
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
        assert (out == SENTINEL).all(), what

    def x(B, K):
        return torch.ones(B, K, device=DEV)

    def w(N, K):
        return torch.ones(N, K, device=DEV, dtype=torch.bfloat16)

    def out(B, N):
        return torch.full((B, N), SENTINEL, device=DEV)

    o = out(1, 1)
    refused(lambda: ops.gemv_bf16(x(1, 32776), w(1, 32776), out=o), o, "B * K = 32776 floats of stage")
    o = out(5, 3)
    refused(lambda: ops.gemv_bf16(x(5, 16), w(3, 16), out=o), o, "B = 5")
    o = out(1, 3)
    refused(lambda: ops.gemv_bf16(x(1, 12), w(3, 12), out=o), o, "K % 8 != 0")
    o = out(1, 2)
    refused(lambda: ops.gemv_bf16(x(1, 16), w(5, 16), out=o, gate_out=True), o, "gate_out with an odd N")
    o = out(1, 3)
    refused(lambda: ops.gemv_bf16(x(1, 16), w(6, 16), out=o, gate_out=True, res=torch.ones(1, 3, device=DEV)), o, "gate_out with a residual")
    o = out(1, 3)
    refused(lambda: ops.gemv_bf16(x(1, 16), w(3, 16), out=o, prologue=ops.PROLOGUE_RMSNORM), o, "RMSNorm without alpha")
    o = out(1, 3)
    xs, ws, gamma = x(1, 16), torch.ones(3, 16, device=DEV), torch.ones(16, device=DEV)
    refused(lambda: _lib.check(_lib.lib().rst_gemv_f32(ops._ptr(xs), ops._ptr(gamma), None, GB.EPS_LN, ops._ptr(ws), None, None, None,
                                                       ops._ptr(o), 1, 3, 16, 0, ops._stream())), o, "LayerNorm gamma without beta")
