"""The weight-only fp8 skinny GEMM (csrc/lm_skinny.hip gemm_skinny_kernel<NB, CT, true>; ops.gemm_skinny_fp8w) on the GPU:

1  the packing launch equals the host restatement (tests/helpers/skinny_fp8w.py) byte for byte, scales in the same order;
2  the product against fp64 on the dequantised weights under the bf16 packed route's per-element bound, on the smallest shapes that
   reach each code path, and deterministic across two calls (the split counters re-arm themselves);
3  ops.lm_gated_pair on fp8 copies (the gate between rows of different scales);
4  agreement with ops.gemm_skinny on the dequantised matrix: bit for bit, the launch plan being the shared one;
5  refusals and the fall-back to the bf16 route;
6  routing: a quantised LMModel above two rows and in prefill streams the fp8 copies and computes the function of the plain model and
   of the CPU oracle on the dequantised state dict."""
import pytest
import torch

from oracle import lm_oracle as L
from rstnet_amd import _lib, ops, synth
from rstnet_amd.lm.model import LMGen, LMModel
from tests.golden import cases
from tests.helpers import lm_fp8w as Q
from tests.helpers import lm_operands as O
from tests.helpers import skinny_fp8w as S
from tests.helpers.gemv_bounds import gate_carry, mixed_rows as _mixed_rows, p_ref as _p_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = Q.U
EPS = 1e-8


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class _profile:
    def __enter__(self):
        self.recs = ops.PROFILE = []
        return self.recs

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        ops.PROFILE = None
        return False


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,interleave", [(33, 64, False), (1001, 704, False), (64, 4096, True)])
def test_pack_weight_equals_the_host_map(N, K, interleave):
    g = torch.Generator().manual_seed(N + K)
    q = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32).to(torch.uint8)        # every byte pattern is copied
    s = torch.exp2(torch.randint(-120, 60, (N,), generator=g).double()).float()
    qp, sp = ops.skinny_pack_weight_fp8w(q.to(DEV), s.to(DEV), interleave_halves=interleave)
    want_q, want_s = S.pack_weight_ref(q, s, interleave)
    assert qp.shape == (S.rows32(N), K) and sp.shape == (S.rows32(N),)
    assert torch.equal(qp.cpu().reshape(-1), want_q)
    assert torch.equal(sp.cpu().view(torch.int32), want_s.view(torch.int32))


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
def _weights(N, K, g):
    """bf16 rows spanning 2^-30 .. 2^30 (so the row scales span 60 binades), row 1 all zero, row 2 of magnitude 2^-104."""
    w = _mixed_rows(N, K, g, -30, 30)
    w[1] = 0
    w[2] = torch.randn(K, generator=g) * 2.0 ** -104
    return w.bfloat16()


# (B, N, K, prologue, res, bias)
CASES = [(3, 1001, 1024, 0, False, False),        # ragged N, one batch tile
         (4, 33, 4096, 1, False, False),          # a second column tile with a single live row
         (5, 96, 8192, 0, True, True),            # K split below 33 rows
         (31, 9001, 288, 2, False, False),        # 18 steps over 8 waves, uneven: waves start on odd steps
         (32, 17001, 512, 1, False, False),       # more column tiles than CUs
         (33, 4099, 4096, 1, False, False),       # two batch tiles, split at K >= 4096
         (64, 4096, 8192, 2, True, False)]        # two batch tiles with a deep split


@pytest.mark.parametrize("B,N,K,mode,res,bias", CASES)
def test_gemm_skinny_fp8w_elementwise_bound(B, N, K, mode, res, bias):
    """|y - y64| <= bound(K, prologue) * (sum_k |P(x)_k| |w_k| + |bias| + |res|) per element, y64 in fp64 on the dequantised weights;
    bound = SPLIT_BOUND + _acc(K) (+ C_PROLOGUE * 2^-24), the bf16 packed route's (helpers.skinny_fp8w.bound).  A row multiplied by a
    neighbour's scale is off by a factor of two or more.  Outputs whose magnitude sum is below 2^-110 (the row of scale < 2^-100 against
    activation rows of 2^-20, which the SiLU-gate prologue squares: results around 2^-137, fp32 subnormals) get the output format's own
    resolution on top (helpers.skinny_fp8w.underflow_floor): measured without it, (31, 9001, 288) read 7550 * 2^-24 there -- a few
    units of 2^-150 against a magnitude of 2^-137 -- while every normal output stays under the relative bound."""
    g = torch.Generator().manual_seed(B * 1000 + N + K)
    x = _mixed_rows(B, 2 * K if mode == 2 else K, g)
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    r = torch.randn(B, N, generator=g) if res else None
    b = torch.randn(N, generator=g) if bias else None
    q, s = ops.quantize_rows_fp8(_weights(N, K, g).to(DEV))
    sc = s.cpu()
    assert not q[1].any() and float(sc[2]) < 2.0 ** -100 and len(set(sc.tolist())) > 20
    split = int(_lib.lib().rst_skinny_bf16_split_plan(B, N, K))
    if (B, N, K) in ((5, 96, 8192), (33, 4099, 4096), (64, 4096, 8192)):
        assert split > 1, "the case is meant to run the in-launch K split"
    dev = lambda t: None if t is None else t.to(DEV)
    run = lambda: ops.gemm_skinny_fp8w(x.to(DEV), q, s, prologue=mode, alpha=dev(alpha) if mode == 1 else None, eps=EPS, res=dev(r), bias=dev(b))
    with _profile() as recs:
        y = run()
    assert [(n, sh) for n, _, _, _, _, sh in recs] == [("gemm_skinny_fp8w", (B, N, K))]
    assert recs[0][4] == N * K + 4 * N + 4 * (x.numel() + B * N)
    y2 = run()
    assert torch.equal(y, y2), "two calls must agree bit for bit (wave-order sums, self re-arming split counters)"
    w64 = Q.dequant_ref(q, s)
    P = _p_ref(x.double(), K, mode, alpha.double())
    ref = P @ w64.t() + (b.double() if bias else 0) + (r.double() if res else 0)
    mag = P.abs() @ w64.abs().t() + (b.double().abs() if bias else 0) + (r.double().abs() if res else 0)
    err = (y.double().cpu() - ref).abs()
    assert not err[:, 1].any() or res or bias, "an all-zero weight row gives exact zeros"
    normal = mag >= 2.0 ** -110          # outputs far above fp32's subnormal range: the relative bound alone
    e = float((err / mag.clamp_min(1e-300))[normal].max())
    tiny = float((err / (S.bound(K, mode) * mag + S.underflow_floor(split)))[~normal].max()) if bool((~normal).any()) else 0.0
    print(f"B={B} N={N} K={K} mode={mode} split={split}: backward error {e / U:.1f} * 2^-24 (bound {S.bound(K, mode) / U:.0f}); "
          f"{int((~normal).sum())} outputs below 2^-110 in magnitude: err / (bound + floor) = {tiny:.3g}")
    assert e <= S.bound(K, mode)
    assert tiny <= 1


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,I,K,bias", [(3, 1408, 512, True), (33, 2816, 4096, False)])
def test_gated_pair_on_fp8_copies(B, I, K, bias):
    """ops.lm_gated_pair with both fp8 copies: res + W_out (silu(u) * v), [u | v] = W_in rmsnorm(x), under the bound of
    tests/test_lm_operands_gpu.py::test_gated_pair_elementwise_bound on the dequantised weights."""
    g = torch.Generator().manual_seed(B + I + K)
    x = _mixed_rows(B, K, g)
    w_in = _mixed_rows(2 * I, K, g, -8, 8) / K ** 0.5
    w_in[0] = torch.randn(K, generator=g) / K ** 0.5        # pair 0 by construction: the v row five binades above the u row
    w_in[I] = torch.randn(K, generator=g) * 32.0 / K ** 0.5
    w_out = _mixed_rows(K, I, g, -8, 8) / I ** 0.5
    q_in, s_in = ops.quantize_rows_fp8(w_in.bfloat16().to(DEV))
    q_out, s_out = ops.quantize_rows_fp8(w_out.bfloat16().to(DEV))
    assert float(s_in[0]) != float(s_in[I]), "u row 0 and v row 0 must carry different scales"
    assert int((s_in[:I] != s_in[I:]).sum()) > I // 2
    b_in = torch.randn(2 * I, generator=g) if bias else torch.zeros(2 * I)
    b_out = torch.randn(K, generator=g) if bias else torch.zeros(K)
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    dev = lambda t: t.to(DEV) if bias else None
    with _profile() as recs:
        y = ops.lm_gated_pair(x.to(DEV), ops.dequantize_rows_fp8(q_in, s_in), ops.dequantize_rows_fp8(q_out, s_out), alpha=alpha.to(DEV),
                              eps=EPS, res=x.to(DEV), bias_in=dev(b_in), bias_out=dev(b_out), w8_in=(q_in, s_in), w8_out=(q_out, s_out))
    assert [(n, sh) for n, _, _, _, _, sh in recs] == [("gemm_skinny_fp8w", (B, 2 * I, K)), ("gemm_skinny_fp8w", (B, K, I))]
    wi, wo = Q.dequant_ref(q_in, s_in), Q.dequant_ref(q_out, s_out)
    P = _p_ref(x.double(), K, 1, alpha.double())
    h = P @ wi.t() + b_in.double()
    dh = S.bound(K, 1) * (P.abs() @ wi.abs().t() + b_in.double().abs())
    gg, dg = gate_carry(h, dh)
    ref = x.double() + gg @ wo.t() + b_out.double()
    g_abs = gg.abs() + dg
    bound = (O.SPLIT_BOUND * g_abs + dg) @ wo.abs().t() + S.acc(I) * (x.double().abs() + b_out.double().abs() + g_abs @ wo.abs().t())
    r = ((y.double().cpu() - ref).abs() / bound).max().item()
    print(f"B={B} I={I} K={K}: max err / bound = {r:.3g}")
    assert r <= 1


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K,mode,res", [(33, 4099, 4096, 1, False), (5, 96, 8192, 0, True), (8, 1001, 2304, 2, False),
                                            (31, 257, 288, 2, False)])
def test_agrees_with_the_bf16_route_bit_for_bit(B, N, K, mode, res):
    """ops.gemm_skinny on dequantize_rows_fp8(q, scale), where it takes the packed form too: K > 2048, and the SiLU-gate prologue at any
    K (288: 18 steps over 8 waves, the fp8 form's waves start on odd steps and share a 16-byte load with their neighbour).  Both routes pack the same activations and
    run the SAME launch plan (rst_skinny_bf16_split_plan, skinny_ct), deal the same steps to the same waves, and differ only in where
    the power-of-two row scale multiplies: it commutes with every fp32 rounding away from underflow (weight rows span 2^-8 .. 2^8
    here), so torch.equal holds -- the stronger of the two statements; agreement within twice the bound is implied and asserted first."""
    g = torch.Generator().manual_seed(B + N + K)
    x = _mixed_rows(B, 2 * K if mode == 2 else K, g, -6, 6).to(DEV)
    alpha = (1 + 0.1 * torch.randn(K, generator=g)).to(DEV) if mode == 1 else None
    r = torch.randn(B, N, generator=g).to(DEV) if res else None
    q, s = ops.quantize_rows_fp8((_mixed_rows(N, K, g, -8, 8) / K ** 0.5).bfloat16().to(DEV))
    w = ops.dequantize_rows_fp8(q, s)
    with _profile() as recs:
        y8 = ops.gemm_skinny_fp8w(x, q, s, prologue=mode, alpha=alpha, eps=EPS, res=r)
        y16 = ops.gemm_skinny(x, w, prologue=mode, alpha=alpha, eps=EPS, res=r)
    assert [n for n, *_ in recs] == ["gemm_skinny_fp8w", "gemm_skinny"]
    P = _p_ref(x.double().cpu(), K, mode, None if alpha is None else alpha.double().cpu())
    mag = P.abs() @ Q.dequant_ref(q, s).abs().t() + (r.double().cpu().abs() if res else 0)
    assert float(((y8.double() - y16.double()).abs().cpu() / mag).max()) <= 2 * S.bound(K, mode)
    assert torch.equal(y8, y16)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_are_refused():
    assert not ops.gemm_skinny_fp8w_supported(8, 64, 272) and not ops.gemm_skinny_fp8w_supported(65, 64, 1024)
    assert ops.gemm_skinny_fp8w_supported(64, 64, 1024)
    s = torch.ones(64, device=DEV)
    with pytest.raises(ValueError):
        ops.gemm_skinny_fp8w(torch.zeros(8, 272, device=DEV), torch.zeros(64, 272, device=DEV, dtype=torch.uint8), s)
    with pytest.raises(ValueError):
        ops.gemm_skinny_fp8w(torch.zeros(65, 1024, device=DEV), torch.zeros(64, 1024, device=DEV, dtype=torch.uint8), s)


def test_lm_linear_falls_back_to_bf16_where_the_shape_is_not_served():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 272, generator=g).to(DEV)
    q, s = ops.quantize_rows_fp8((torch.randn(96, 272, generator=g) / 16).bfloat16().to(DEV))
    w = ops.dequantize_rows_fp8(q, s)
    with _profile() as recs:
        y = ops.lm_linear(x, w, w8=(q, s))
    assert [(n, sh) for n, _, _, _, _, sh in recs] == [("gemm_skinny", (8, 96, 272))]
    assert torch.equal(y, ops.lm_linear(x, w))


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def _tiny(weight_dtype="fp8", cfg=None):
    cfg = dict(cfg or synth.LM_TINY)
    sd = synth.lm_state_dict(cfg, cases.LM_SEED)
    model = LMModel.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, cfg).quantize_weights_(weight_dtype)
    return cfg, model


def _fp32_cpu(sd):
    return {k: v.detach().cpu().float() for k, v in sd.items()}


def _layer_shapes(cfg, B, Hd):
    E = cfg["dim"]
    return [(B, 3 * E, E), (B, E, E), (B, 2 * Hd, E), (B, E, Hd)] * cfg["num_layers"]


def test_quantised_step_at_batch_8_streams_the_fp8_copies():
    cfg, model = _tiny()
    B, E, Hd = 8, cfg["dim"], 704
    toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, 1), generator=torch.Generator().manual_seed(5)).to(DEV)
    with model.streaming(B):
        with _profile() as recs:
            model.forward_text(toks)
    got = [r[5] for r in recs if r[0] == "gemm_skinny_fp8w"]
    assert got == _layer_shapes(cfg, B, Hd) + [(B, cfg["text_card"], E)], got
    covered = {(n, k) for _, n, k in got}
    assert not [r for r in recs if r[0] == "gemm_skinny" and (r[5][1], r[5][2]) in covered]
    assert not [r for r in recs if r[0] == "gemv_fp8w"]


def test_quantised_batch_8_equals_the_plain_model_and_the_oracle():
    """13 steps, the 10-slot ring wraps: out and logits within rel_err < 1e-3 (the project's model-level tolerance) of a plain bf16
    LMModel holding the dequantised state dict and of the CPU oracle on it."""
    cfg, model = _tiny()
    B = 8
    plain = LMModel.from_state_dict({k: v.clone() for k, v in model.state_dict().items()}, cfg)
    assert plain.weight_dtype == "bf16"
    ocfg = L.LMConfig(**cfg)
    sdf = _fp32_cpu(model.state_dict())
    st = L.new_transformer_state(B, ocfg.num_layers, ocfg.num_heads, ocfg.dim // ocfg.num_heads, ocfg.context)
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    with model.streaming(B), plain.streaming(B):
        for s in range(13):
            toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, 1), generator=g)
            toks[0, 2, 0] = -1
            with _profile() as recs:
                out, logits = model.forward_text(toks.to(DEV))
            assert [r[0] for r in recs].count("gemm_skinny_fp8w") == 4 * cfg["num_layers"] + 1
            p_out, p_logits = plain.forward_text(toks.to(DEV))
            o_out, o_logits = L.forward_text(sdf, ocfg, toks, st)
            e = max(rel_err(out, p_out), rel_err(logits, p_logits), rel_err(out, o_out), rel_err(logits, o_logits))
            assert e < 1e-3, f"step {s}: {e:.3g}"
            worst = max(worst, e)
    print(f"LM_TINY fp8 B=8: max rel_err over 13 steps = {worst:.3g}")


@pytest.mark.parametrize("graphs", [False, True])
def test_lmgen_greedy_tokens_at_batch_4_match_the_oracle(graphs, monkeypatch):
    monkeypatch.setenv("NO_CUDA_GRAPH", "0" if graphs else "1")
    cfg, model = _tiny()
    B = 4
    user = cases.lm_user_tokens(cfg, batch=B)
    og = L.LMGenOracle(_fp32_cpu(model.state_dict()), L.LMConfig(**cfg), B)
    gen = LMGen(model, use_sampling=False)
    with gen.streaming(B):
        for s in range(cases.LM_STEPS):
            o = gen.step(user[s].to(DEV))
            ref = og.step(user[s])
            assert (o is None) == (ref is None), s
            if o is not None:
                assert torch.equal(o.cpu(), ref), (s, o.cpu().flatten().tolist(), ref.flatten().tolist())


def test_prefill_of_70_frames_streams_fp8_and_equals_the_stepped_session():
    """LMGen.prefill of T = 70 recorded frames of 7 streams: seven turns of the 10-slot ring, one pass of 10 positions per turn (a pass
    is never longer than the ring), i.e. 70 rows per linear = one 64-row chunk and a tail of 6.  The stepped session provides the
    recording; after the prefill the following steps return its tokens."""
    cfg, model = _tiny()
    T, after, B = 70, 4, 7
    gen = LMGen(model, use_sampling=False)
    F = T + gen.max_delay + after
    user = cases.lm_user_tokens(cfg, steps=F, batch=B)
    with gen.streaming(B):
        stepped = [gen.step(user[f].to(DEV)) for f in range(F)]
    assert all(o is None for o in stepped[:gen.max_delay]) and all(o is not None for o in stepped[gen.max_delay:])
    own = gen.model_time(torch.cat(stepped[gen.max_delay:], -1))
    users = torch.cat(list(user), -1).to(DEV)
    gen = LMGen(model, use_sampling=False)
    with gen.streaming(B):
        with _profile() as recs:
            assert gen.prefill(users[:, :, :T], own[:, :, :T]) is None
        names = [r[0] for r in recs]
        assert "gemm_skinny_fp8w" in names and "gemm_skinny" not in names, sorted(set(names))
        rows = {r[5][0] for r in recs if r[0] == "gemm_skinny_fp8w"}
        assert rows == {64, 6}, rows
        for f in range(T, F):
            o = gen.step(user[f].to(DEV))
            assert o is not None and torch.equal(o, stepped[f]), f"frame {f}"


def test_one_real_layer_at_batch_32_builds_no_bf16_packed_copy():
    cfg = dict(synth.LM_MOSHI_7B, num_layers=1)
    B = 32
    model = LMModel.from_state_dict(synth.lm_state_dict(cfg, seed=4, device=DEV), cfg).quantize_weights_("fp8")
    plain = LMModel.from_state_dict({k: v.clone() for k, v in model.state_dict().items()}, cfg)
    for c in (ops._skinny_weights, ops._skinny_weights_gated):
        c.clear()
    g = torch.Generator().manual_seed(5)
    worst, outs = 0.0, []
    with model.streaming(B):
        for s in range(3):
            toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, 1), generator=g).to(DEV)
            with _profile() as recs:
                outs.append((toks, *model.forward_text(toks)))
            assert [r[0] for r in recs].count("gemm_skinny_fp8w") == 5 and not [r for r in recs if r[0] == "gemm_skinny"]
    keys = set(ops._skinny_weights._d) | set(ops._skinny_weights_gated._d)
    for mod, name in model._covered_weights():
        w = getattr(mod, name)
        assert (w.device, w.data_ptr(), tuple(w.shape), w.dtype) not in keys, f"a bf16 packed copy of a {tuple(w.shape)} matrix was built"
    with plain.streaming(B):
        for toks, out, logits in outs:
            ref_out, ref_logits = plain.forward_text(toks)
            worst = max(worst, rel_err(out, ref_out), rel_err(logits, ref_logits))
    print(f"LM_MOSHI_7B, one layer, B=32: max rel_err over 3 steps = {worst:.3g}")
    assert worst < 1e-3


def test_mxfp4_model_at_batch_8_keeps_bf16_layers_and_an_fp8_head():
    cfg, model = _tiny("mxfp4")
    B, E, Hd = 8, cfg["dim"], 704
    plain = LMModel.from_state_dict({k: v.clone() for k, v in model.state_dict().items()}, cfg)
    toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, 1), generator=torch.Generator().manual_seed(5)).to(DEV)
    with model.streaming(B), plain.streaming(B):
        with _profile() as recs:
            out, logits = model.forward_text(toks)
        ref_out, ref_logits = plain.forward_text(toks)
    assert [r[5] for r in recs if r[0] == "gemm_skinny"] == _layer_shapes(cfg, B, Hd)
    assert [r[5] for r in recs if r[0] == "gemm_skinny_fp8w"] == [(B, cfg["text_card"], E)]
    assert rel_err(out, ref_out) < 1e-3 and rel_err(logits, ref_logits) < 1e-3
