"""The weight-only MXFP4 skinny GEMM (csrc/lm_skinny.hip gemm_skinny_kernel<NB, CT, false, true>; ops.gemm_skinny_mxfp4w) on the GPU:

1  the packing launch equals the host restatement (tests/helpers/skinny_mxfp4w.py) byte for byte, codes and scale bytes;
2  the decode, exhaustively: every code under every scale byte the quantiser can emit, read out through one-hot activations;
3  the product against fp64 on the dequantised weights under the bf16 packed route's per-element bound, on the smallest shapes that
   reach each code path, and deterministic across two calls (the split counters re-arm themselves);
4  agreement with ops.gemm_skinny on the dequantised matrix: bit for bit, unconditionally (no scale touches an accumulator);
5  ops.lm_gated_pair on two opted-in copies;
6  refusals and the fall-back to the bf16 route;
7  routing: an LMModel from quantize_weights_("mxfp4", batched=True) above two rows and in prefill streams the MXFP4 copies and computes
   the function of the plain model and of the CPU oracle on the dequantised state dict."""
import pytest
import torch

from oracle import lm_oracle as L
from rstnet_amd import _lib, ops, synth
from rstnet_amd.lm.model import LMGen, LMModel
from tests.golden import cases
from tests.helpers import lm_mxfp4 as Q4
from tests.helpers import lm_operands as O
from tests.helpers import skinny_fp8w as S8
from tests.helpers import skinny_mxfp4w as S
from tests.helpers.gemv_bounds import gate_carry, mixed_rows as _mixed_rows, p_ref as _p_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = Q4.U
EPS = 1e-8
NAME = "gemm_skinny_mxfp4w"


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
    q = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(torch.uint8)        # every byte pattern is only copied
    s = torch.randint(0, 256, (N, K // 32), generator=g, dtype=torch.int32).to(torch.uint8)
    qp, sp = ops.skinny_pack_weight_mxfp4w(q.to(DEV), s.to(DEV), interleave_halves=interleave)
    want_q, want_s = S.pack_weight_ref(q, s, interleave)
    assert qp.shape == (S.rows32(N), K // 2) and sp.shape == (S.rows32(N) // 32, K // 32, 32)
    assert qp.dtype == sp.dtype == torch.uint8
    assert torch.equal(qp.cpu().reshape(-1), want_q)
    assert torch.equal(sp.cpu().reshape(-1), want_s)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,block", [(32, 0), (64, 1)])
def test_decode_of_every_code_under_every_scale_byte(K, block):
    """q and scale built by hand (helpers.skinny_mxfp4w.exhaustive_codes): one row per scale byte 2 .. 245, all 16 codes twice in block
    ``block``; x = the 32 one-hot rows of that block.  y[b][n] is then w[n][32 * block + b] times 1.0 plus zeros: exact, so an inexact
    convert, a wrong nibble or (K = 64) a neighbour's scale shows as a differing bit."""
    q, s = S.exhaustive_codes(K, block)
    w = ops.dequantize_blocks_mxfp4(q, s)
    x = torch.zeros(32, K)
    x[torch.arange(32), 32 * block + torch.arange(32)] = 1.0
    y = ops.gemm_skinny_mxfp4w(x.to(DEV), q.to(DEV), s.to(DEV)).cpu()
    want = w.float()[:, 32 * block:32 * block + 32].t().contiguous()
    assert y.shape == (32, 244)
    bad = (y.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert torch.equal(y, want), f"{len(bad)} differ; first (b, n) = {bad[0].tolist()}: got {float(y[tuple(bad[0])])!r}, want {float(want[tuple(bad[0])])!r}"


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K,mode,res,bias", S.BOUND_CASES)
def test_gemm_skinny_mxfp4w_elementwise_bound(B, N, K, mode, res, bias):
    """|y - y64| <= bound(K, prologue) * (sum_k |P(x)_k| |w_k| + |bias| + |res|) per element, y64 in fp64 on the dequantised weights;
    bound = helpers.skinny_fp8w.bound, the bf16 packed route's, imported.  Block magnitudes are drawn independently over +-15 binades
    (helpers.skinny_mxfp4w.block_weights), so a block decoded with a neighbour's scale is off by a factor of two or more.  No underflow
    floor: tests/test_skinny_mxfp4w_cpu.py::test_the_bound_cases_stay_in_the_normal_range holds every magnitude sum of these inputs at or
    above 2^-110, except the all-zero weight row, which must give exact zeros."""
    x, alpha, r, b, w = S.bound_inputs(B, N, K, mode, res, bias)
    q, s = ops.quantize_blocks_mxfp4(w.to(DEV))
    assert not q[1].any() and len(set(s.flatten().tolist())) > 20
    split = int(_lib.lib().rst_skinny_bf16_split_plan(B, N, K))
    if (B, N, K) in ((5, 96, 8192), (33, 4099, 4096), (64, 4096, 8192)):
        assert split > 1, "the case is meant to run the in-launch K split"
    dev = lambda t: None if t is None else t.to(DEV)
    run = lambda: ops.gemm_skinny_mxfp4w(x.to(DEV), q, s, prologue=mode, alpha=dev(alpha) if mode == 1 else None, eps=EPS, res=dev(r), bias=dev(b))
    with _profile() as recs:
        y = run()
    assert [(n, sh) for n, _, _, _, _, sh in recs] == [(NAME, (B, N, K))]
    assert recs[0][4] == N * K // 2 + N * K // 32 + 4 * (x.numel() + B * N)
    y2 = run()
    assert torch.equal(y, y2), "two calls must agree bit for bit (wave-order sums, self re-arming split counters)"
    w64 = Q4.dequant_ref(q, s)
    P = _p_ref(x.double(), K, mode, alpha.double())
    ref = P @ w64.t() + (b.double() if bias else 0) + (r.double() if res else 0)
    mag = P.abs() @ w64.abs().t() + (b.double().abs() if bias else 0) + (r.double().abs() if res else 0)
    assert bool(torch.isfinite(ref).all())
    err = (y.double().cpu() - ref).abs()
    live = mag > 0
    if not (res or bias):
        assert not y[:, 1].any(), "an all-zero weight row gives exact zeros"
        assert not live[:, 1].any() and bool(live[:, 0].all()) and bool(live[:, 2:].all())
    else:
        assert bool(live.all())
    assert float(mag[live].min()) >= 2.0 ** -110
    e = float((err[live] / mag[live]).max())
    print(f"B={B} N={N} K={K} mode={mode} split={split}: backward error {e / U:.1f} * 2^-24 (bound {S8.bound(K, mode) / U:.0f})")
    assert not err[~live].any()
    assert e <= S8.bound(K, mode)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K,mode,res", [(33, 4099, 4096, 1, False), (5, 96, 8192, 0, True), (8, 1001, 2304, 2, False),
                                            (31, 257, 288, 2, False)])
def test_agrees_with_the_bf16_route_bit_for_bit(B, N, K, mode, res):
    """ops.gemm_skinny on dequantize_blocks_mxfp4(q, scale), where it takes the packed form too (K > 2048, and the SiLU-gate prologue at
    any K; 288 = 18 steps over 8 waves: waves of the MXFP4 form start on odd steps and share an 8-byte load with their neighbour).  Both
    routes pack the same activations, run the SAME launch plan and feed the SAME bf16 operand to the same MFMAs in the same order: no
    scale touches an accumulator, so torch.equal holds whatever the magnitudes (blocks span +-15 binades here)."""
    g = torch.Generator().manual_seed(B + N + K)
    x = _mixed_rows(B, 2 * K if mode == 2 else K, g, -6, 6).to(DEV)
    alpha = (1 + 0.1 * torch.randn(K, generator=g)).to(DEV) if mode == 1 else None
    r = torch.randn(B, N, generator=g).to(DEV) if res else None
    q, s = ops.quantize_blocks_mxfp4(S.block_weights(N, K, g).to(DEV))
    w = ops.dequantize_blocks_mxfp4(q, s)
    with _profile() as recs:
        y4 = ops.gemm_skinny_mxfp4w(x, q, s, prologue=mode, alpha=alpha, eps=EPS, res=r)
        y16 = ops.gemm_skinny(x, w, prologue=mode, alpha=alpha, eps=EPS, res=r)
    assert [n for n, *_ in recs] == [NAME, "gemm_skinny"]
    assert torch.equal(y4, y16)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,I,K,bias", [(3, 1408, 512, True), (33, 2816, 4096, False)])
def test_gated_pair_on_opted_in_copies(B, I, K, bias):
    """ops.lm_gated_pair with both copies opted in: res + W_out (silu(u) * v), [u | v] = W_in rmsnorm(x): exactly the two MXFP4 launches,
    values under the bound of tests/test_skinny_fp8w_gpu.py::test_gated_pair_on_fp8_copies on the dequantised weights."""
    g = torch.Generator().manual_seed(B + I + K)
    x = _mixed_rows(B, K, g)
    w_in = _mixed_rows(2 * I, K, g, -8, 8) / K ** 0.5
    w_in[0] = torch.randn(K, generator=g) / K ** 0.5        # pair 0 by construction: the v row five binades above the u row
    w_in[I] = torch.randn(K, generator=g) * 32.0 / K ** 0.5
    w_out = _mixed_rows(K, I, g, -8, 8) / I ** 0.5
    c_in = ops.Mxfp4BatchedCopy(*ops.quantize_blocks_mxfp4(w_in.bfloat16().to(DEV)))
    c_out = ops.Mxfp4BatchedCopy(*ops.quantize_blocks_mxfp4(w_out.bfloat16().to(DEV)))
    assert int(c_in.scale[0, 0]) != int(c_in.scale[I, 0]), "u row 0 and v row 0 must carry different scales"
    b_in = torch.randn(2 * I, generator=g) if bias else torch.zeros(2 * I)
    b_out = torch.randn(K, generator=g) if bias else torch.zeros(K)
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    dev = lambda t: t.to(DEV) if bias else None
    with _profile() as recs:
        y = ops.lm_gated_pair(x.to(DEV), ops.dequantize_blocks_mxfp4(*c_in), ops.dequantize_blocks_mxfp4(*c_out), alpha=alpha.to(DEV),
                              eps=EPS, res=x.to(DEV), bias_in=dev(b_in), bias_out=dev(b_out), w8_in=c_in, w8_out=c_out)
    assert [(n, sh) for n, _, _, _, _, sh in recs] == [(NAME, (B, 2 * I, K)), (NAME, (B, K, I))]
    wi, wo = Q4.dequant_ref(*c_in), Q4.dequant_ref(*c_out)
    P = _p_ref(x.double(), K, 1, alpha.double())
    h = P @ wi.t() + b_in.double()
    dh = S8.bound(K, 1) * (P.abs() @ wi.abs().t() + b_in.double().abs())
    gg, dg = gate_carry(h, dh)
    ref = x.double() + gg @ wo.t() + b_out.double()
    g_abs = gg.abs() + dg
    bound = (O.SPLIT_BOUND * g_abs + dg) @ wo.abs().t() + S8.acc(I) * (x.double().abs() + b_out.double().abs() + g_abs @ wo.abs().t())
    r = ((y.double().cpu() - ref).abs() / bound).max().item()
    print(f"B={B} I={I} K={K}: max err / bound = {r:.3g}")
    assert r <= 1


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_are_refused():
    assert not ops.gemm_skinny_mxfp4w_supported(8, 64, 272) and not ops.gemm_skinny_mxfp4w_supported(65, 64, 1024)
    assert ops.gemm_skinny_mxfp4w_supported(64, 64, 1024)
    with pytest.raises(ValueError):
        ops.gemm_skinny_mxfp4w(torch.zeros(8, 272, device=DEV), torch.zeros(64, 136, device=DEV, dtype=torch.uint8),
                               torch.full((64, 8), 127, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.gemm_skinny_mxfp4w(torch.zeros(65, 1024, device=DEV), torch.zeros(64, 512, device=DEV, dtype=torch.uint8),
                               torch.full((64, 32), 127, device=DEV, dtype=torch.uint8))


def test_lm_linear_falls_back_to_bf16_where_the_shape_is_not_served():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 272, generator=g).to(DEV)
    w = (torch.randn(96, 272, generator=g) / 16).bfloat16().to(DEV)
    copy = ops.Mxfp4BatchedCopy(torch.zeros(96, 136, device=DEV, dtype=torch.uint8), torch.full((96, 8), 127, device=DEV, dtype=torch.uint8))
    with _profile() as recs:
        y = ops.lm_linear(x, w, w8=copy)
    assert [(n, sh) for n, _, _, _, _, sh in recs] == [("gemm_skinny", (8, 96, 272))]
    assert torch.equal(y, ops.lm_linear(x, w))


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------
def _tiny(batched=True, cfg=None):
    cfg = dict(cfg or synth.LM_TINY)
    sd = synth.lm_state_dict(cfg, cases.LM_SEED)
    model = LMModel.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, cfg).quantize_weights_("mxfp4", batched=batched)
    return cfg, model


def _fp32_cpu(sd):
    return {k: v.detach().cpu().float() for k, v in sd.items()}


def _layer_shapes(cfg, B, Hd):
    E = cfg["dim"]
    return [(B, 3 * E, E), (B, E, E), (B, 2 * Hd, E), (B, E, Hd)] * cfg["num_layers"]


def test_opted_in_step_at_batch_8_streams_the_mxfp4_copies():
    cfg, model = _tiny()
    assert model.weight_dtype == "mxfp4" and model.mxfp4_batched is True
    B, E, Hd = 8, cfg["dim"], 704
    toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, 1), generator=torch.Generator().manual_seed(5)).to(DEV)
    with model.streaming(B):
        with _profile() as recs:
            model.forward_text(toks)
    assert [r[5] for r in recs if r[0] == NAME] == _layer_shapes(cfg, B, Hd)
    assert [r[5] for r in recs if r[0] == "gemm_skinny_fp8w"] == [(B, cfg["text_card"], E)]
    covered = {(n, k) for _, n, k in _layer_shapes(cfg, B, Hd)} | {(cfg["text_card"], E)}
    assert not [r for r in recs if r[0] == "gemm_skinny" and (r[5][1], r[5][2]) in covered]
    assert not [r for r in recs if r[0] == "gemv_mxfp4w"]


def test_opted_in_batch_8_equals_the_plain_model_and_the_oracle():
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
            assert [r[0] for r in recs].count(NAME) == 4 * cfg["num_layers"]
            p_out, p_logits = plain.forward_text(toks.to(DEV))
            o_out, o_logits = L.forward_text(sdf, ocfg, toks, st)
            e = max(rel_err(out, p_out), rel_err(logits, p_logits), rel_err(out, o_out), rel_err(logits, o_logits))
            assert e < 1e-3, f"step {s}: {e:.3g}"
            worst = max(worst, e)
    print(f"LM_TINY mxfp4 batched B=8: max rel_err over 13 steps = {worst:.3g}")


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


def test_prefill_of_70_frames_streams_mxfp4_and_equals_the_stepped_session():
    """LMGen.prefill of T = 70 recorded frames of 7 streams: one pass of 10 positions per turn of the 10-slot ring, i.e. 70 rows per
    linear = one 64-row chunk and a tail of 6.  The stepped session provides the recording; after the prefill the following steps
    return its tokens."""
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
        assert NAME in names and "gemm_skinny" not in names, sorted(set(names))
        rows = {r[5][0] for r in recs if r[0] == NAME}
        assert rows == {64, 6}, rows
        for f in range(T, F):
            o = gen.step(user[f].to(DEV))
            assert o is not None and torch.equal(o, stepped[f]), f"frame {f}"


def test_switching_the_route_on_later_keeps_the_codes():
    cfg, model = _tiny(batched=False)
    assert model.mxfp4_batched is False
    stored = [(m, n, getattr(m, n + "_q4"), getattr(m, n + "_s4")) for m, n in model._layer_weights()]
    saved = [(q.clone(), s.clone()) for _, _, q, s in stored]
    assert model.quantize_weights_("mxfp4", batched=True) is model and model.mxfp4_batched is True and model.weight_dtype == "mxfp4"
    for (m, n, q, s), (q0, s0) in zip(stored, saved):
        assert getattr(m, n + "_q4") is q and getattr(m, n + "_s4") is s and torch.equal(q, q0) and torch.equal(s, s0)
    B, Hd = 8, 704
    toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, 1), generator=torch.Generator().manual_seed(5)).to(DEV)
    with model.streaming(B):
        with _profile() as recs:
            model.forward_text(toks)
    assert [r[5] for r in recs if r[0] == NAME] == _layer_shapes(cfg, B, Hd)
    with pytest.raises(ValueError):
        model.quantize_weights_("fp8", batched=True)


def test_one_real_layer_at_batch_32_builds_no_bf16_packed_copy():
    cfg = dict(synth.LM_MOSHI_7B, num_layers=1)
    B = 32
    model = LMModel.from_state_dict(synth.lm_state_dict(cfg, seed=4, device=DEV), cfg, weight_dtype="mxfp4", batched=True)
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
            names = [r[0] for r in recs]
            assert names.count(NAME) == 4 and names.count("gemm_skinny_fp8w") == 1 and "gemm_skinny" not in names
    keys = set(ops._skinny_weights._d) | set(ops._skinny_weights_gated._d)
    for mod, name in model._layer_weights():
        w = getattr(mod, name)
        assert (w.device, w.data_ptr(), tuple(w.shape), w.dtype) not in keys, f"a bf16 packed copy of a {tuple(w.shape)} matrix was built"
    with plain.streaming(B):
        for toks, out, logits in outs:
            ref_out, ref_logits = plain.forward_text(toks)
            worst = max(worst, rel_err(out, ref_out), rel_err(logits, ref_logits))
    print(f"LM_MOSHI_7B, one layer, B=32: max rel_err over 3 steps = {worst:.3g}")
    assert worst < 1e-3
