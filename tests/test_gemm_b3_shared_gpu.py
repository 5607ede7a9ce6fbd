"""The window-sharing form of the three-plane conv GEMMs (gemm_win_b3_stream_shared_kernel: a tile stages every group of S * C activations
once and multiplies it for all R = 2 / 3 taps, tiles 128 - (R - 1) output rows apart, never across utterances) against fp64 references,
through RF.conv1d / RF.convtr1d, with the bounds of tests/test_gemm_b3_gpu.py: the backward error max |y - y64| / sum |x||w| below
1.25 x the f32 instruction's + 2^-24 and below 16 x 2^-24, and 2e-6 of the reference's scale for the fused-epilogue cases."""
import pytest
import torch
import torch.nn.functional as F

from oracle import mimi_oracle as O
from rstnet_amd import ops, synth
from rstnet_amd.codec import functional as RF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def nlc(t):
    return t.transpose(1, 2).contiguous().to(DEV)


def _profiled(fn):
    ops.PROFILE = []
    try:
        out = fn()
        names = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    return out, names


def _conv_ref64(x, w, stride):
    """Causal conv (left pad k - stride, right pad to a whole last window) in fp64 on the device, as windows x weights: the value and
    sum |x||w|, both [B, T_out, Cout]."""
    B, cin, T = x.shape
    cout, _, k = w.shape
    t_out = -(-T // stride)
    xp = F.pad(x.double().to(DEV), (k - stride, (t_out - 1) * stride + stride - T))
    win = xp.unfold(2, k, stride).permute(0, 2, 1, 3).reshape(B * t_out, cin * k)        # [rows][ci][tap]
    wm = w.double().to(DEV).reshape(cout, cin * k)
    return (win @ wm.t()).view(B, t_out, cout), (win.abs() @ wm.abs().t()).view(B, t_out, cout)


def _check_backward_error(run, ref, bound, monkeypatch):
    """run() on the three-plane route (profiled name asserted) and on the f32 instruction; the bounds of the module docstring."""
    monkeypatch.setattr(ops, "GEMM_B3", True)
    y3, names = _profiled(run)
    assert names == ["gemm_win_b3"]
    monkeypatch.setattr(ops, "GEMM_B3", False)
    y1 = run()
    monkeypatch.setattr(ops, "GEMM_B3", True)
    assert y3.shape == ref.shape
    e3 = float(((y3.double() - ref).abs() / bound).max())
    e1 = float(((y1.double() - ref).abs() / bound).max())
    print(f"backward error / 2^-24: three-plane {e3 / U:.2f}, f32 instruction {e1 / U:.2f}")
    assert e3 < 1.25 * e1 + U
    assert e3 < 16 * U


def _wide_range(g, *shape):
    return torch.randn(*shape, generator=g) * torch.exp(torch.randn(*shape, generator=g))


@pytest.mark.parametrize("B,cin,cout,k,s,T", [
    (3, 16, 80, 8, 4, 5999),           # S * C = 64, ragged N (128-wide tiles), T % s != 0, T_out = 1500 (% 127 != 0), M = 4500
    (2, 64, 256, 8, 4, 131075),        # 128 x 256 tiles: 513 of them, T % s != 0
    (3, 16, 80, 4, 2, 3001),           # S * C = 32: not eligible, today's kernel
    (5, 64, 128, 7, 1, 1017),          # R = 7: not eligible, today's kernel
], ids=["r2_strided", "r2_wide", "not_eligible_g32", "not_eligible_k7"])
def test_shared_strided_conv_backward_error(B, cin, cout, k, s, T, monkeypatch):
    g = torch.Generator().manual_seed(B + cin + T)
    x = _wide_range(g, B, cin, T)
    w = synth._xavier(g, cout, cin, k)
    ref, bound = _conv_ref64(x, w, s)
    xd, wd = nlc(x), RF.pack_conv_weight(w).to(DEV)
    _check_backward_error(lambda: RF.conv1d(xd, wd, None, k_eff=k, stride=s), ref, bound, monkeypatch)


@pytest.mark.parametrize("B,cin,cout,s,T", [(3, 64, 32, 4, 1500), (3, 128, 64, 5, 1500)], ids=["N128", "N320"])
def test_shared_transposed_conv_backward_error(B, cin, cout, s, T, monkeypatch):
    g = torch.Generator().manual_seed(cin + s)
    k = 2 * s
    x = _wide_range(g, B, cin, T)
    w = torch.randn(cin, cout, k, generator=g) / (2 * cin) ** 0.5
    ref = O.causal_convtr1d(x.double(), w.double(), None, stride=s).transpose(1, 2).to(DEV)
    bound = O.causal_convtr1d(x.double().abs(), w.double().abs(), None, stride=s).transpose(1, 2).to(DEV)
    xd, wd = nlc(x), RF.pack_convtr_weight(w, s).to(DEV)
    _check_backward_error(lambda: RF.convtr1d(xd, wd, None, kernel=k, stride=s), ref, bound, monkeypatch)


@pytest.mark.parametrize("B,T", [(40, 110), (5, 1016), (5, 1017), (5, 1008), (5, 1009)])
def test_shared_k3_conv_with_fused_epilogue(B, T):
    """k3 64 -> 128 with ELU on load, bias, residual and ELU out.  40 x 110: every tile has padding rows at both ends; 1016 / 1017 and
    1008 / 1009 (= 8 x 126, the tile step of three taps): the row limit around a tile edge."""
    g = torch.Generator().manual_seed(B * T)
    cin, cout = 64, 128
    x = torch.rand(B, cin, T, generator=g) * 4 - 2
    w = synth._xavier(g, cout, cin, 3)
    b = 0.1 * torch.randn(cout, generator=g)
    res = torch.randn(B, cout, T, generator=g)
    y, names = _profiled(lambda: RF.conv1d(nlc(x), RF.pack_conv_weight(w).to(DEV), b.to(DEV), k_eff=3, act_in=ops.ACT_ELU, res=nlc(res),
                                           act_out=ops.ACT_ELU_OUT))
    assert names == ["gemm_win_b3"]
    ref = F.elu(res.double() + F.conv1d(F.pad(F.elu(x.double()), (2, 0)), w.double(), b.double()))
    err = float((y.transpose(1, 2).double().cpu() - ref).abs().max() / ref.abs().max())
    assert err < 2e-6, err


@pytest.mark.parametrize("B,cin,cout,k,s,T,frames", [
    (5, 64, 128, 3, 1, 1017, ((1, 126), (3, 1016))),       # first row of the second tile (windows in two tiles); the last frame
    (3, 16, 80, 8, 4, 5999, ((0, 3), (2, 5998))),          # inside the first group; in the partial last group
], ids=["k3", "strided"])
def test_shared_non_finite_frames_reach_their_rows_only(B, cin, cout, k, s, T, frames):
    """One inf and one NaN activation: exactly the output rows whose windows contain the frame are non-finite, all others are
    bit-equal to the clean run -- nothing leaks through the shifted fragment reads, the cleared rows or the dead accumulator rows."""
    g = torch.Generator().manual_seed(k + s)
    x = torch.randn(B, cin, T, generator=g)
    wd = RF.pack_conv_weight(synth._xavier(g, cout, cin, k)).to(DEV)
    clean, names = _profiled(lambda: RF.conv1d(nlc(x), wd, None, k_eff=k, stride=s))
    assert names == ["gemm_win_b3"] and bool(torch.isfinite(clean).all())
    xb = x.clone()
    hit = torch.zeros(B, clean.shape[1], dtype=torch.bool)
    t = torch.arange(clean.shape[1])
    for (b, f), v in zip(frames, (float("inf"), float("nan"))):
        xb[b, (7 * f) % cin, f] = v
        hit[b] |= (t * s - (k - s) <= f) & (f < t * s - (k - s) + k)
    assert 0 < int(hit.sum()) <= 2 * k
    y, names = _profiled(lambda: RF.conv1d(nlc(xb), wd, None, k_eff=k, stride=s))
    assert names == ["gemm_win_b3"]
    y, clean = y.cpu(), clean.cpu()
    assert not torch.isfinite(y[hit]).any()
    assert torch.equal(y[~hit], clean[~hit])
