"""Weight-only fp8 (e4m3fn, one power-of-two scale per row) storage of the small-batch LM step, on the GPU:

3  the device quantiser (rst_quant_rows_fp8) is bit-identical, bytes and scales, to the host restatement (tests/helpers/lm_fp8w.py);
4  the GEMV decodes every finite byte code exactly, at every byte position of a 16-byte load;
5  rst_gemv_fp8w_f32 against fp64 on the dequantised weights under a per-element backward-error bound derived from the kernel's own
   summation structure (helpers.lm_fp8w.c_gemv), every covered Moshi-7B matrix and ragged shapes;
6  the quantised LMModel computes the function of a plain bf16 LMModel loaded with the dequantised state dict;
7  ... and of the CPU oracle fed the dequantised weights: logits, and greedy LMGen token streams identical;
8  host logic: idempotence, state_dict, B = 8, no persistent temporal launch, the profile of an eager frame, quantising in a session;
9  StreamingPipeline with a quantised LM against the composed oracles.

Mutations built once while writing these tests (each in a scratch copy of the kernels, all three schedules; the scale now
multiplies in `sum` of the two schedules of csrc/lm_gemv_quant.h and in the K-split epilogue of csrc/lm_gemv_fp8.hip): applying row
0's scale to every row fails every case of test_gemv_fp8w_elementwise_bound and test_decode_table; scaling the bias as well
(``(acc + bias) * scale``) fails every case of test_gemv_fp8w_elementwise_bound that has a bias."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import lm_oracle as L
from oracle import mimi_oracle as MO
from rstnet_amd import ops, synth
from rstnet_amd.codec.mimi import MimiCodec
from rstnet_amd.lm.model import LMGen, LMModel
from rstnet_amd.pipeline import StreamingPipeline
from tests.golden import cases
from tests.helpers import lm_fp8w as Q
from tests.helpers.gemv_bounds import gate_carry, mixed_rows as _mixed_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = Q.U
EPS = 1e-8


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
def _assert_same_quantisation(w: torch.Tensor):
    q, s = ops.quantize_rows_fp8(w.to(DEV))
    q_ref, s_ref = Q.quant_rows_ref(w)
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32)), "scales differ"
    bad = (q.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, [(int(n), int(k), float(w[n, k]), int(q[n, k]), int(q_ref[n, k])) for n, k in bad[:8]]
    return q, s


def test_device_quantiser_on_hand_picked_rows():
    w, exps, want = Q.special_rows()
    q, s = _assert_same_quantisation(w.bfloat16())
    assert torch.equal(s.cpu().double(), torch.exp2(exps.double()))
    for r, codes in want.items():
        assert q[r, :len(codes)].tolist() == codes
    d = ops.dequantize_rows_fp8(q, s)
    assert d.dtype == torch.bfloat16 and torch.equal(d.cpu().double(), Q.dequant_ref(q, s))


@pytest.mark.parametrize("N,K", [(12288, 4096), (4096, 11264), (1001, 704), (5, 16), (37, 2816), (3, 7)])
def test_device_quantiser_matches_host(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = (_mixed_rows(N, K, g, -12, 12) / K ** 0.5).bfloat16()
    if N > 2:
        w[1] = 0
    sp, _, _ = Q.special_rows(K) if K >= 32 else (torch.zeros(0, K), None, None)
    n = min(sp.shape[0], N - 2) if N > 2 else 0
    if n > 0:
        w[2:2 + n] = sp[:n].bfloat16()
    _assert_same_quantisation(w)


def test_quantiser_refuses_non_finite():
    w = torch.ones(4, 32, dtype=torch.bfloat16, device=DEV)
    w[2, 5] = float("inf")
    with pytest.raises(ValueError):
        ops.quantize_rows_fp8(w)
    w[2, 5] = float("nan")
    with pytest.raises(ValueError):
        ops.quantize_rows_fp8(w)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def _code_matrix(N, K):
    q = ((torch.arange(N)[:, None] + torch.arange(K)[None, :]) % 256).to(torch.uint8)
    q[(q & 0x7F) == 0x7F] = 0                      # the two NaN codes are never produced
    return q


@pytest.mark.parametrize("N,K,ks", [(256, 256, list(range(16)) + [255]), (4096, 4096, [5, 1029, 4095])])
def test_decode_table(N, K, ks):
    """One-hot x: y[n] = value(q[n, k]) * s_n exactly, for all 254 finite codes (every column of the code matrix holds them all), every
    byte position of a 16-byte load, two scales; the small case runs the LDS-staged schedule, the large one the K-split one."""
    q = _code_matrix(N, K)
    s = torch.where(torch.arange(N) % 2 == 0, 2.0 ** -3, 2.0 ** 5).float()
    val = Q.fp8_value(q) * s.double()[:, None]
    qd, sd = q.to(DEV), s.to(DEV)
    seen = set()
    for k in ks:
        x = torch.zeros(1, K)
        x[0, k] = 1.0
        y = ops.gemv_fp8w(x.to(DEV), qd, sd).cpu().double()
        assert torch.equal(y[0], val[:, k]), k
        seen |= set(q[:, k].tolist())
    assert len(seen - {0x7F, 0xFF}) == 254


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def _p_ref(x64, K, mode, alpha64):
    if mode == 1:
        return x64 * alpha64 / torch.sqrt(float(np.float32(EPS)) + (x64 * x64).mean(dim=1, keepdim=True))
    if mode == 2:
        return F.silu(x64[:, :K]) * x64[:, K:]
    return x64


# (N, K, prologue, res, gate_out, bias)
REAL = [(12288, 4096, 1, False, False, False), (4096, 4096, 0, True, False, False), (22528, 4096, 1, False, True, False),
        (4096, 11264, 0, True, False, False), (32000, 4096, 0, False, False, False), (8192, 4096, 0, False, False, False),
        (12288, 4096, 1, True, False, True), (22528, 4096, 1, False, True, True), (4096, 11264, 0, True, False, True)]
RAGGED = [(N, K, (N + K) % 3, N != 37, False, K != 704) for N in (5, 37, 1001) for K in (16, 704, 2816)]
GATED = [(2816, 704, 1, False, True, True), (10, 16, 1, False, True, True), (2002, 2816, 0, False, True, True)]
CASES = ([(B,) + c for c in REAL[:6] + RAGGED + GATED for B in (1, 2)] + [(1,) + c for c in REAL[6:]]
         + [(B, 1001, 2816, m, True, False, True) for B in (3, 4) for m in (0, 2)])


@pytest.mark.parametrize("B,N,K,mode,res,gate,bias", CASES)
def test_gemv_fp8w_elementwise_bound(B, N, K, mode, res, gate, bias):
    """|y - y64| <= (c + c_P) * 2^-24 * (sum_k |w_k P(x)_k| + |bias| + |res|) per element, y64 in fp64 on the dequantised weights.

    c = helpers.lm_fp8w.c_gemv(K) = 16 * ceil(K / 1024) + 12: the longest fmaf chain of a lane (16 per 1024-wide chunk), the 6-step
    butterfly, the 3 cross-wave additions of the K-split schedule, bias and residual, and one unit for the second-order term (derived
    there).  c_P = 32 with a prologue: the fp32 error of RMSNorm / the SiLU gate relative to |P(x)|, the bound
    tests/test_lm_operands_gpu.py states (C_PROLOGUE).  gate_out: the same bound on u and v, carried through silu(u) * v to first order
    (|silu'| < 1.1) plus 8 roundings for the fp32 silu and the product.
    Weight rows span 2^-8 .. 2^8, so their scales span 17 powers of two: a row multiplied by another row's scale is off by a factor
    of two or more, and a bias multiplied by the scale is off by |bias| |s - 1|, both orders of magnitude beyond the bound."""
    g = torch.Generator().manual_seed(B * 1000 + N + K + mode)
    x = _mixed_rows(B, 2 * K if mode == 2 else K, g, -6, 6)
    w = (_mixed_rows(N, K, g, -8, 8) / K ** 0.5).bfloat16()
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    No = N // 2 if gate else N
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(B, No, generator=g) if res else None
    dev = lambda t: None if t is None else t.to(DEV)
    q, s = ops.quantize_rows_fp8(w.to(DEV))
    assert len(set(s.cpu().tolist())) >= 2, "the rows must not share one scale"
    y = ops.gemv_fp8w(x.to(DEV), q, s, prologue=mode, alpha=dev(alpha) if mode == 1 else None, eps=EPS, res=dev(r), bias=dev(b),
                      gate_out=gate).cpu().double()
    assert y.shape == (B, No)
    w64 = Q.dequant_ref(q, s)
    P = _p_ref(x.double(), K, mode, alpha.double())
    b64 = b.double() if bias else torch.zeros(N, dtype=torch.float64)
    h = P @ w64.t() + b64
    c = (Q.c_gemv(K) + (Q.C_PROLOGUE if mode else 0)) * U
    dh = c * (P.abs() @ w64.abs().t() + b64.abs())
    if mode == 2:       # the fp32 silu(u) = u / (1 + expf(-u)) is -0 where expf(-u) overflows (u < -88.7): there |silu(u)| < 2^-121
        dh = dh + (x[:, K:].double().abs() * 2.0 ** -120) @ w64.abs().t()
    if gate:
        ref, bound = gate_carry(h, dh)
    else:
        ref = h + (r.double() if res else 0)
        bound = dh + (c * r.double().abs() if res else 0)
    ratio = ((y - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"B={B} N={N} K={K} mode={mode} res={res} gate={gate} bias={bias}: max err / bound = {ratio:.3g} (c = {c / U:.0f})")
    assert ratio <= 1


def test_gemv_fp8w_unsupported_shapes_are_refused():
    x = torch.zeros(1, 24, device=DEV)
    q = torch.zeros(8, 24, device=DEV, dtype=torch.uint8)
    s = torch.ones(8, device=DEV)
    assert not ops.gemv_fp8w_supported(1, 8, 24)
    with pytest.raises(ValueError):
        ops.gemv_fp8w(x, q, s)


# ---- 6 .. 8: the model ------------------------------------------------------------------------------------------------------------------
def _tiny(cfg=None):
    cfg = dict(cfg or synth.LM_TINY)
    sd = synth.lm_state_dict(cfg, cases.LM_SEED)
    model = LMModel.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, cfg)
    return cfg, sd, model


def _fp32_cpu(sd):
    return {k: v.detach().cpu().float() for k, v in sd.items()}


def test_quantize_weights_host_logic():
    cfg, sd, model = _tiny()
    assert model.weight_dtype == "bf16"
    assert model.quantize_weights_("fp8") is model and model.weight_dtype == "fp8"
    want, covered = Q.quantise_state_dict(sd, cfg)
    got = model.state_dict()
    assert set(got.keys()) == set(sd.keys()), "the fp8 copies are not part of the state dict"
    for k in sd:
        assert torch.equal(got[k].cpu(), want[k]), k
        assert (k in covered) or torch.equal(got[k].cpu(), sd[k])
    changed = sum(not torch.equal(want[k], sd[k]) for k in covered)
    assert changed == len(covered)
    # idempotent: the copies are kept, the parameters are not written again
    ptrs = [(getattr(m, n + "_q8").data_ptr(), getattr(m, n)._version) for m, n in model._covered_weights()]
    assert model.quantize_weights_("fp8") is model
    assert ptrs == [(getattr(m, n + "_q8").data_ptr(), getattr(m, n)._version) for m, n in model._covered_weights()]
    # the copy of a weight that is written afterwards is dropped: that linear goes back to the bf16 route
    from rstnet_amd.lm.model import _w8
    assert _w8(model.text_linear) is not None
    model.text_linear.weight.mul_(2)
    assert _w8(model.text_linear) is None
    with pytest.raises(ValueError):
        model.quantize_weights_("int4")
    with pytest.raises(ValueError):
        model.quantize_weights_("bf16")
    m2 = LMModel.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, cfg, weight_dtype="fp8")
    assert m2.weight_dtype == "fp8" and torch.equal(m2.text_linear.weight.cpu(), want["text_linear.weight"])


def test_quantize_weights_refuses_non_finite():
    cfg, sd, model = _tiny()
    before = model.transformer.layers[0].self_attn.in_proj_weight.clone()
    model.transformer.layers[1].gating.linear_out.weight[3, 3] = float("nan")
    with pytest.raises(ValueError):
        model.quantize_weights_("fp8")
    assert model.weight_dtype == "bf16" and torch.equal(model.transformer.layers[0].self_attn.in_proj_weight, before)


def test_quantising_inside_a_live_session_raises():
    """A captured frame graph embeds the bf16 weights' pointers and would go on streaming them: quantising while a session is open
    raises; after the session it works."""
    cfg, sd, model = _tiny()
    gen = LMGen(model, use_sampling=False)
    user = cases.lm_user_tokens(cfg)
    with gen.streaming(cases.LM_BATCH):
        for s in range(4):
            gen.step(user[s].to(DEV))
        with pytest.raises(RuntimeError):
            model.quantize_weights_("fp8")
    assert model.weight_dtype == "bf16"
    model.quantize_weights_("fp8")


def _route_equivalence(cfg, seed, B, steps):
    sd = synth.lm_state_dict(cfg, seed=seed, device=DEV)
    model = LMModel.from_state_dict(sd, cfg).quantize_weights_("fp8")
    plain = LMModel.from_state_dict({k: v.clone() for k, v in model.state_dict().items()}, cfg)
    assert plain.weight_dtype == "bf16"
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    with model.streaming(B), plain.streaming(B):
        for s in range(steps):
            toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, 1), generator=g).to(DEV)
            recs = []
            ops.PROFILE = recs
            try:
                out, logits = model.forward_text(toks)
            finally:
                ops.PROFILE = None
            names = [r[0] for r in recs]
            assert names.count("gemv_fp8w") == 4 * cfg["num_layers"] + 1 and "gemv_bf16" not in names, names
            ref_out, ref_logits = plain.forward_text(toks)
            worst = max(worst, rel_err(out, ref_out), rel_err(logits, ref_logits))
    return worst


@pytest.mark.parametrize("B", [1, 2])
def test_route_equivalence_tiny(B):
    """Quantised model vs a plain bf16 LMModel holding the dequantised values: the same function in a different summation order.  Per
    GEMV the two differ by at most 2 c 2^-24 sum |w x| (test 5's bound, both routes), c <= 188; through two layers that stays orders
    below the project's model-level tolerance rel_err < 1e-3, which is what is asserted."""
    e = _route_equivalence(dict(synth.LM_TINY), cases.LM_SEED, B, 13)
    print(f"LM_TINY B={B}: max rel_err over 13 steps = {e:.3g}")
    assert e < 1e-3


def test_route_equivalence_one_real_layer():
    e = _route_equivalence(dict(synth.LM_MOSHI_7B, num_layers=1), 4, 1, 3)
    print(f"LM_MOSHI_7B, one layer, B=1: max rel_err over 3 steps = {e:.3g}")
    assert e < 1e-3


@pytest.mark.parametrize("B", [cases.LM_BATCH, 8])
def test_logits_match_oracle_on_dequantised_weights(B):
    """forward_text / forward_depformer against the CPU oracle fed the quantised model's state dict, 13 steps (the 10-slot ring wraps).
    B = 8 runs the skinny-GEMM route on the bf16 parameters, which hold the same values."""
    cfg, sd, model = _tiny()
    model.quantize_weights_("fp8")
    ocfg = L.LMConfig(**cfg)
    sdf = _fp32_cpu(model.state_dict())
    gt = torch.Generator().manual_seed(5)
    st = L.new_transformer_state(B, ocfg.num_layers, ocfg.num_heads, ocfg.dim // ocfg.num_heads, ocfg.context)
    with model.streaming(B):
        for s in range(13):
            toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, 1), generator=gt)
            toks[0, 2, 0] = -1
            ref_out, ref_logits = L.forward_text(sdf, ocfg, toks, st)
            recs = []
            ops.PROFILE = recs
            try:
                out, logits = model.forward_text(toks.to(DEV))
            finally:
                ops.PROFILE = None
            assert ("gemv_fp8w" in [r[0] for r in recs]) == (B <= 2)
            assert rel_err(out, ref_out) < 1e-3 and rel_err(logits, ref_logits) < 1e-3, f"step {s}"
            dst = L.new_transformer_state(B, ocfg.depformer_num_layers, ocfg.depformer_num_heads,
                                          ocfg.depformer_dim // ocfg.depformer_num_heads, ocfg.dep_q)
            model.depformer._streaming_state = model.depformer._init_streaming_state(B)
            prev = torch.randint(0, cfg["text_card"], (B, 1, 1), generator=gt)
            for cb in range(cfg["dep_q"]):
                rl = L.forward_depformer(sdf, ocfg, cb, prev, ref_out, dst)
                gl = model.forward_depformer(cb, prev.to(DEV), out)
                assert rel_err(gl, rl) < 1e-3, f"step {s} cb {cb}"
                prev = torch.randint(0, cfg["card"], (B, 1, 1), generator=gt)


@pytest.mark.parametrize("graphs,depth_frame", [(False, True), (True, True), (False, False), (True, False)])
def test_lmgen_greedy_tokens_match_oracle_on_dequantised_weights(graphs, depth_frame, monkeypatch):
    """Greedy LMGen.step of the quantised model == LMGenOracle on its state dict, token for token, with and without HIP graphs and with the
    depth phase as persistent launch and as chain.  (Not against lm_tiny.npz: on random weights quantisation legitimately moves tokens.)"""
    monkeypatch.setenv("NO_CUDA_GRAPH", "0" if graphs else "1")
    monkeypatch.setenv("RST_DEPTH_FRAME", "1" if depth_frame else "0")
    cfg, sd, model = _tiny()
    model.quantize_weights_("fp8")
    user = cases.lm_user_tokens(cfg)
    B = cases.LM_BATCH
    og = L.LMGenOracle(_fp32_cpu(model.state_dict()), L.LMConfig(**cfg), B)
    gen = LMGen(model, use_sampling=False)
    with gen.streaming(B):
        for s in range(cases.LM_STEPS):
            o = gen.step(user[s].to(DEV))
            ref = og.step(user[s])
            assert (o is None) == (ref is None), s
            if o is not None:
                assert torch.equal(o.cpu(), ref), (s, o.cpu().flatten().tolist(), ref.flatten().tolist())


def test_eager_frame_profile_shows_every_covered_gemv_as_fp8(monkeypatch):
    monkeypatch.setenv("NO_CUDA_GRAPH", "1")
    cfg, sd, model = _tiny()
    model.quantize_weights_("fp8")
    gen = LMGen(model, use_sampling=False)
    user = cases.lm_user_tokens(cfg, batch=1)
    recs = []
    with gen.streaming(1):
        gen.step(user[0].to(DEV))
        ops.PROFILE = recs
        try:
            gen.step(user[1].to(DEV))
            torch.cuda.synchronize()
        finally:
            ops.PROFILE = None
    shapes = sorted(r[5] for r in recs if r[0] == "gemv_fp8w")
    E, Hd, Ed = cfg["dim"], 704, cfg["depformer_dim"]
    want = sorted([(1, 3 * E, E), (1, E, E), (1, 2 * Hd, E), (1, E, Hd)] * cfg["num_layers"] + [(1, cfg["text_card"], E), (1, cfg["dep_q"] * Ed, E)])
    assert shapes == want, shapes
    covered = {(n, k) for _, n, k in want}
    assert not [r for r in recs if r[0] == "gemv_bf16" and (r[5][1], r[5][2]) in covered]
    for r in recs:
        if r[0] == "gemv_fp8w":
            _, N, K = r[5]
            assert r[4] == N * K + 4 * N + 4 * (K + (N // 2 if N == 2 * Hd else N))


def test_no_persistent_temporal_launch_for_a_quantised_model():
    """Past 2048 ring steps a bf16 batch-1 session moves to the persistent temporal launch (and re-captures its frame); a quantised one
    must not: that launch reads the bf16 weights."""
    cfg = dict(synth.LM_MOSHI_7B, num_layers=1)
    model = LMModel.from_state_dict(synth.lm_state_dict(cfg, seed=4, device=DEV), cfg)
    model.quantize_weights_("fp8")
    gen = LMGen(model, use_sampling=False)
    g = torch.Generator().manual_seed(3)
    user = torch.randint(0, cfg["card"], (8, 1, cfg["n_q"] - cfg["dep_q"], 1), generator=g).to(DEV)
    with gen.streaming(1):
        st = model.transformer._streaming_state
        st.pos.fill_(2044)
        st.offset_cpu = 2044
        graphs = set()
        for s in range(8):                      # crosses ops.TEMPORAL_FRAME_AUTO_POS
            gen.step(user[s])
            graphs.add(id(gen._streaming_state.graphed_frame))
        assert st.offset_cpu == 2052 and ops.temporal_frame_wanted(st.offset_cpu)
        assert st.tables is None, "the persistent temporal launch built its tables"
        assert len(graphs) == 1 and gen._streaming_state.temporal_choice is False, "the frame was re-captured at 2048"
        recs = []
        ops.PROFILE = recs
        try:
            model.forward_text(torch.zeros(1, cfg["n_q"] + 1, 1, dtype=torch.long, device=DEV))
            torch.cuda.synchronize()
        finally:
            ops.PROFILE = None
        assert [r[0] for r in recs].count("gemv_fp8w") == 5 and not [r for r in recs if r[0] in ("gemv_bf16", "temporal_frame")]


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------
def test_streaming_pipeline_with_a_quantised_lm_matches_composed_oracles():
    B, frames = 2, 6
    cfg = dict(synth.LM_TINY_16Q)
    mimi_sd = synth.mimi_state_dict(0)
    lm_sd = synth.lm_state_dict(cfg, seed=9)
    mimi = MimiCodec.from_state_dict(mimi_sd).to(DEV)
    model = LMModel.from_state_dict({k: v.to(DEV) for k, v in lm_sd.items()}, cfg, weight_dtype="fp8")
    gen = LMGen(model, use_sampling=False)
    pcm = synth.synth_audio(B, frames * 1920, seed=21)
    outs = []
    with StreamingPipeline(mimi, gen, B) as pipe:
        for f in range(frames):
            outs.append(pipe.step(pcm[:, :, f * 1920:(f + 1) * 1920].contiguous().to(DEV)))
        fused = pipe._fused is not None and not pipe._fused.disable
    assert fused, "the last frames must have run as the fused end-to-end graph"
    assert outs[0] is None and all(o is not None and o.shape == (B, 1, 1920) for o in outs[1:])
    got = torch.cat([o.cpu() for o in outs[1:]], -1)
    mcfg = MO.MimiConfig()
    with torch.no_grad():
        codes = MO.encode(mimi_sd, mcfg, pcm)
        og = L.LMGenOracle(_fp32_cpu(model.state_dict()), L.LMConfig(**cfg), B)
        toks = [og.step(codes[:, :, f:f + 1]) for f in range(frames)]
        gen_codes = torch.cat([t[:, 1:] for t in toks[1:]], -1)
        ref = MO.decode(mimi_sd, mcfg, gen_codes)
    assert got.shape == ref.shape
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"pipeline waveform rel_err = {err:.3g}")
    assert err < 1e-3, err
    # the tokens themselves (the pipeline hands out the waveform only): the same LMGen fed the oracle encoder's codes
    n_user = cfg["n_q"] - cfg["dep_q"]
    with gen.streaming(B):
        for f in range(frames):
            o = gen.step(codes[:, :n_user, f:f + 1].contiguous().to(DEV))
            assert (o is None) == (toks[f] is None)
            if o is not None:
                assert torch.equal(o.cpu(), toks[f]), f
