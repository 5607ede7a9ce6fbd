"""Weight-only MXFP4 (e2m1 codes, one power-of-two scale byte per block of 32 k) storage of the small-batch LM step, on the GPU:

1  the device quantiser (rst_quant_blocks_mxfp4) is bit-identical, codes and scale bytes, to the host restatement
   (tests/helpers/lm_mxfp4.py);
2  the GEMV decodes all 16 codes exactly at every one of the 32 nibble positions of a 16-byte load, with each block's own scale, in
   every schedule the launcher can pick;
3  rst_gemv_mxfp4w_f32 against fp64 on the dequantised weights under a per-element backward-error bound derived from the kernel's own
   summation structure (helpers.lm_mxfp4.c_gemv), every covered Moshi-7B per-layer matrix and ragged shapes;
4  unsupported shapes raise;
5  the model: host logic, route equivalence against a plain bf16 LMModel on the dequantised state dict, the CPU oracle fed the
   dequantised weights (logits, greedy LMGen tokens), no persistent temporal launch, StreamingPipeline.

Mutations built once while writing these tests (each in a scratch copy of the kernels, every schedule; scale byte and nibble order
now live in W4Chunk of csrc/lm_gemv_fp4.hip, the bias in the epilogues of csrc/lm_gemv_quant.h): block 0's
scale byte for every block of a row fails every case of test_decode_table and every case of test_gemv_mxfp4w_elementwise_bound with
more than one block per row (the eight K = 32 cases pass, as they must); swapped nibbles (the two weights of a byte exchanged) fail
every case of both; the scale applied to the bias as well (``bias * 2^e`` of the row's first block) fails every case of
test_gemv_mxfp4w_elementwise_bound that has a bias and none of the others."""
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
from tests.helpers import lm_mxfp4 as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = Q.U
EPS = 1e-8


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _mixed_rows(rows, cols, g, lo, hi):
    """randn rows scaled by 2^e, e uniform in [lo, hi] (row 0 at the low end, the last row at the high end)."""
    e = torch.randint(lo, hi + 1, (rows,), generator=g)
    e[0], e[-1] = lo, hi
    return torch.randn(rows, cols, generator=g) * torch.exp2(e.double()).float()[:, None]


def _mixed_blocks(N, K, g, lo, hi):
    """randn [N, K] with every block of 32 k scaled by 2^e, e uniform in [lo, hi]; within each row the first block sits at the low end
    and the last at the high end (one block: the high end), so neighbouring blocks' scales differ by many binades."""
    e = torch.randint(lo, hi + 1, (N, K // 32, 1), generator=g)
    e[:, 0], e[:, -1] = lo, hi
    return (torch.randn(N, K // 32, 32, generator=g) * torch.exp2(e.double()).float()).view(N, K)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
def _assert_same_quantisation(w: torch.Tensor):
    q, s = ops.quantize_blocks_mxfp4(w.to(DEV))
    q_ref, s_ref = Q.quant_blocks_ref(w)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and q.shape == q_ref.shape and s.shape == s_ref.shape
    bad = (s.cpu() != s_ref).nonzero()
    assert bad.numel() == 0, ("scale bytes differ", [(int(n), int(j), int(s[n, j]), int(s_ref[n, j])) for n, j in bad[:8]])
    bad = (q.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, [(int(n), int(j), float(w[n, 2 * j]), float(w[n, 2 * j + 1]), hex(int(q[n, j])), hex(int(q_ref[n, j]))) for n, j in bad[:8]]
    return q, s


def test_device_quantiser_on_hand_picked_blocks():
    w, exps, want = Q.special_blocks()
    q, s = _assert_same_quantisation(w.bfloat16())
    assert torch.equal(s.cpu()[:, 0].long() - 127, exps)
    codes = Q.codes_of(q)
    for r, c in want.items():
        assert codes[r, :len(c)].tolist() == c
    d = ops.dequantize_blocks_mxfp4(q, s)
    assert d.dtype == torch.bfloat16 and torch.equal(d.cpu().double(), Q.dequant_ref(q, s))


@pytest.mark.parametrize("N,K", [(5, 32), (37, 2816), (1001, 704), (4096, 11264), (12288, 4096)])
def test_device_quantiser_matches_host(N, K):
    """Blocks of very different magnitude inside every row (2^-12 .. 2^12), a zero row, the hand-picked blocks."""
    g = torch.Generator().manual_seed(N + K)
    w = (_mixed_blocks(N, K, g, -12, 12) / K ** 0.5).bfloat16()
    w[1] = 0
    sp, _, _ = Q.special_blocks()
    n = min(sp.numel(), K)
    w[2, :n] = sp.flatten()[:n].bfloat16()
    _assert_same_quantisation(w)


@pytest.mark.parametrize("bad", [float("inf"), float("nan"), 2.0 ** 121])
def test_quantiser_refusals(bad):
    w = torch.ones(4, 64, dtype=torch.bfloat16, device=DEV)
    w[2, 5] = bad
    with pytest.raises(ValueError):
        ops.quantize_blocks_mxfp4(w)
    with pytest.raises(ValueError):
        ops.quantize_blocks_mxfp4(torch.ones(4, 48, dtype=torch.bfloat16, device=DEV))


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
def _code_matrix(N, K):
    """Byte (n + j) % 256 at [n, j]: every nibble column holds all 16 codes within 256 rows.  Scale bytes alternate between 2^-3 and 2^5
    along the blocks of a row, starting with the row's parity."""
    q = ((torch.arange(N)[:, None] + torch.arange(K // 2)[None, :]) % 256).to(torch.uint8)
    s = torch.where((torch.arange(N)[:, None] + torch.arange(K // 32)[None, :]) % 2 == 0, 127 - 3, 127 + 5).to(torch.uint8)
    return q, s


# the smallest shape that takes each schedule of rst_launch_gemv_mxfp4w: LDS-staged (one wave-load per row; four, through the two-in-flight
# loop); whole rows per wave (N * K = 2^24 at the longest and at a short K)
DECODE = [(256, 256, list(range(32)) + [37, 255]), (64, 8192, [5, 2048 + 33, 6000, 8191]), (4096, 4096, [5, 1029, 2048 + 63, 4095]),
          (8192, 2048, [7, 1000, 2047])]


@pytest.mark.parametrize("N,K,ks", DECODE)
def test_decode_table(N, K, ks):
    """One-hot x: y[n] = value(code[n, k]) * 2^e[n, k / 32] exactly, for all 16 codes (every nibble column of the code matrix holds
    them all) at every one of the 32 nibble positions of a 16-byte load (the small case), two scale bytes alternating inside every
    row: a wrong nibble order, a neighbouring block's scale or a wrong stage permutation each change some y."""
    q, s = _code_matrix(N, K)
    assert K < 64 or len(set(s[0].tolist())) == 2
    val = Q.dequant_ref(q, s)
    qd, sd = q.to(DEV), s.to(DEV)
    seen = set()
    for k in ks:
        x = torch.zeros(1, K)
        x[0, k] = 1.0
        y = ops.gemv_mxfp4w(x.to(DEV), qd, sd).cpu().double()
        bad = (y[0] != val[:, k]).nonzero().flatten()
        assert bad.numel() == 0, (k, [(int(n), float(y[0, n]), float(val[n, k])) for n in bad[:8]])
        seen |= set(Q.codes_of(q)[:, k].tolist())
    assert seen == set(range(16))


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
def _p_ref(x64, K, mode, alpha64):
    if mode == 1:
        return x64 * alpha64 / torch.sqrt(float(np.float32(EPS)) + (x64 * x64).mean(dim=1, keepdim=True))
    if mode == 2:
        return F.silu(x64[:, :K]) * x64[:, K:]
    return x64


# (N, K, prologue, res, gate_out, bias)
# the four covered per-layer matrices of Moshi-7B with their real prologue / residual / gate: in_proj, out_proj, gating.linear_in,
# gating.linear_out (K = 11264 is 5.5 wave-loads: the last one is partial), then the same with a bias
REAL = [(12288, 4096, 1, False, False, False), (4096, 4096, 0, True, False, False), (22528, 4096, 1, False, True, False),
        (4096, 11264, 0, True, False, False),
        (12288, 4096, 1, True, False, True), (22528, 4096, 1, False, True, True), (4096, 11264, 0, True, False, True)]
# whole rows per wave at the smallest N * K that takes them, a short K (one wave-load per row), with and without the norm
PATHS = [(8192, 2048, 0, True, False, True), (16384, 1024, 1, False, False, True)]
RAGGED = [(N, K, (N + K) % 3, N != 37, False, K != 704) for N in (5, 37, 1001) for K in (32, 704, 2816)]
GATED = [(2816, 704, 1, False, True, True), (10, 32, 1, False, True, True), (2002, 2816, 0, False, True, True)]
CASES = ([(1,) + c for c in REAL + PATHS] + [(B,) + c for c in RAGGED + GATED for B in (1, 2)]
         + [(B, 1001, 2816, m, True, False, True) for B in (3, 4) for m in (0, 2)]
         + [(2, 64, 11264, 2, True, False, True)])          # the LDS-staged schedule with a partial last wave-load


@pytest.mark.parametrize("B,N,K,mode,res,gate,bias", CASES)
def test_gemv_mxfp4w_elementwise_bound(B, N, K, mode, res, gate, bias):
    """|y - y64| <= (c + c_P) * 2^-24 * (sum_k |w_k P(x)_k| + |bias| + |res|) per element, y64 in fp64 on the dequantised weights.

    c = helpers.lm_mxfp4.c_gemv(K) = 17 * ceil(K / 2048) + 9 (derived there).  c_P = 32 with a prologue: the fp32 error of RMSNorm /
    the SiLU gate relative to |P(x)|, the bound tests/test_lm_operands_gpu.py states (C_PROLOGUE).  gate_out: the same bound on u and
    v, carried through silu(u) * v to first order (|silu'| < 1.1) plus 8 roundings for the fp32 silu and the product.
    The blocks of every weight row span 2^-9 .. 2^9 (19 binades, the first block at the low end, the last at the high end): a block
    multiplied by a neighbour's scale is off by a factor the bound cannot absorb, and so is a bias that meets a scale."""
    g = torch.Generator().manual_seed(B * 1000 + N + K + mode)
    x = _mixed_rows(B, 2 * K if mode == 2 else K, g, -6, 6)
    w = (_mixed_blocks(N, K, g, -9, 9) / K ** 0.5).bfloat16()
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    No = N // 2 if gate else N
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(B, No, generator=g) if res else None
    dev = lambda t: None if t is None else t.to(DEV)
    q, s = ops.quantize_blocks_mxfp4(w.to(DEV))
    if K >= 64:
        sc = s.cpu().long()
        assert int((sc.amax(dim=1) - sc.amin(dim=1)).min()) >= 16, "the blocks of every row must span >= 16 binades"
    y = ops.gemv_mxfp4w(x.to(DEV), q, s, prologue=mode, alpha=dev(alpha) if mode == 1 else None, eps=EPS, res=dev(r), bias=dev(b),
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
        I = N // 2
        u, v, du, dv = h[:, :I], h[:, I:], dh[:, :I], dh[:, I:]
        ref = F.silu(u) * v
        bound = 1.1 * (v.abs() + dv) * du + F.silu(u).abs() * dv + 8 * U * ref.abs() + v.abs() * 2.0 ** -110
    else:
        ref = h + (r.double() if res else 0)
        bound = dh + (c * r.double().abs() if res else 0)
    ratio = ((y - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"B={B} N={N} K={K} mode={mode} res={res} gate={gate} bias={bias}: max err / bound = {ratio:.3g} (c = {c / U:.0f})")
    assert ratio <= 1


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def test_gemv_mxfp4w_unsupported_shapes_are_refused():
    assert not ops.gemv_mxfp4w_supported(1, 8, 48) and not ops.gemv_mxfp4w_supported(5, 8, 64) and not ops.gemv_mxfp4w_supported(4, 8, 11264)
    with pytest.raises(ValueError):
        ops.gemv_mxfp4w(torch.zeros(5, 64, device=DEV), torch.zeros(8, 32, device=DEV, dtype=torch.uint8),
                        torch.full((8, 2), 127, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.gemv_mxfp4w(torch.zeros(4, 11264, device=DEV), torch.zeros(8, 5632, device=DEV, dtype=torch.uint8),
                        torch.full((8, 352), 127, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.gemv_mxfp4w(torch.zeros(1, 64, device=DEV), torch.zeros(8, 32, device=DEV, dtype=torch.uint8),
                        torch.full((8, 2), 127, device=DEV, dtype=torch.uint8), res=torch.zeros(1, 4, device=DEV), gate_out=True)


# ---- 5: the model -----------------------------------------------------------------------------------------------------------------------
def _tiny(cfg=None):
    cfg = dict(cfg or synth.LM_TINY)
    sd = synth.lm_state_dict(cfg, cases.LM_SEED)
    model = LMModel.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, cfg)
    return cfg, sd, model


def _fp32_cpu(sd):
    return {k: v.detach().cpu().float() for k, v in sd.items()}


def test_quantize_weights_host_logic():
    from rstnet_amd.lm.model import _w4, _w8
    cfg, sd, model = _tiny()
    assert model.weight_dtype == "bf16"
    assert model.quantize_weights_("mxfp4") is model and model.weight_dtype == "mxfp4" and model.transformer.weight_dtype == "mxfp4"
    want, as4, as8 = Q.quantise_state_dict(sd, cfg)
    assert len(as4) == 4 * cfg["num_layers"] and len(as8) == 1 + cfg["dep_q"]
    got = model.state_dict()
    assert set(got.keys()) == set(sd.keys()), "the quantised copies are not part of the state dict"
    for k in sd:
        assert torch.equal(got[k].cpu(), want[k]), k
        assert (k in as4) or (k in as8) or torch.equal(got[k].cpu(), sd[k])
    assert sum(not torch.equal(want[k], sd[k]) for k in as4 + as8) == len(as4 + as8)
    # the per-layer matrices hold MXFP4 copies and no fp8 ones; the heads the reverse
    layer = list(model._layer_weights())
    heads = [(model.text_linear, "weight")] + [(m, "weight") for m in model.depformer_in]
    for m, n in layer:
        c = _w4(m, n)
        w = getattr(m, n)
        assert c is not None and _w8(m, n) is None
        assert c[0].dtype == torch.uint8 and c[0].shape == (w.shape[0], w.shape[1] // 2) and c[1].shape == (w.shape[0], w.shape[1] // 32)
    for m, n in heads:
        assert _w8(m, n) is not None and _w4(m, n) is None
    assert model.depformer_in_all_w8() is not None
    # idempotent: the copies are kept, the parameters are not written again
    snap = lambda: [(getattr(m, n + "_q4").data_ptr(), getattr(m, n)._version) for m, n in layer] + \
                   [(getattr(m, n + "_q8").data_ptr(), getattr(m, n)._version) for m, n in heads]
    ptrs = snap()
    assert model.quantize_weights_("mxfp4") is model and ptrs == snap()
    # the copy of a weight that is written afterwards is dropped: that linear goes back to the bf16 route
    out_proj = model.transformer.layers[0].self_attn.out_proj
    assert _w4(out_proj) is not None
    out_proj.weight.mul_(2)
    assert _w4(out_proj) is None
    for name in ("int4", "bf16", "fp8"):
        with pytest.raises(ValueError):
            model.quantize_weights_(name)
    m2 = LMModel.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, cfg, weight_dtype="mxfp4")
    k0 = "transformer.layers.0.gating.linear_in.weight"
    assert m2.weight_dtype == "mxfp4" and torch.equal(m2.state_dict()[k0].cpu(), want[k0])
    m3 = LMModel.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, cfg, weight_dtype="fp8")
    with pytest.raises(ValueError):
        m3.quantize_weights_("mxfp4")
    assert m3.weight_dtype == "fp8"


@pytest.mark.parametrize("bad", [float("nan"), 2.0 ** 121])
def test_quantize_weights_refuses_bad_values(bad):
    cfg, sd, model = _tiny()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.transformer.layers[1].gating.linear_out.weight[3, 3] = bad
    before["transformer.layers.1.gating.linear_out.weight"][3, 3] = bad
    with pytest.raises(ValueError):
        model.quantize_weights_("mxfp4")
    assert model.weight_dtype == "bf16" and model.transformer.weight_dtype == "bf16"
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k].view(torch.int16) if v.dtype == torch.bfloat16 else after[k],
                           v.view(torch.int16) if v.dtype == torch.bfloat16 else v), k


def test_quantising_inside_a_live_session_raises():
    cfg, sd, model = _tiny()
    gen = LMGen(model, use_sampling=False)
    user = cases.lm_user_tokens(cfg)
    with gen.streaming(cases.LM_BATCH):
        for s in range(4):
            gen.step(user[s].to(DEV))
        with pytest.raises(RuntimeError):
            model.quantize_weights_("mxfp4")
    assert model.weight_dtype == "bf16"
    model.quantize_weights_("mxfp4")


def _route_equivalence(cfg, seed, B, steps):
    sd = synth.lm_state_dict(cfg, seed=seed, device=DEV)
    model = LMModel.from_state_dict(sd, cfg).quantize_weights_("mxfp4")
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
            assert names.count("gemv_mxfp4w") == 4 * cfg["num_layers"] and names.count("gemv_fp8w") == 1 and "gemv_bf16" not in names, names
            ref_out, ref_logits = plain.forward_text(toks)
            worst = max(worst, rel_err(out, ref_out), rel_err(logits, ref_logits))
    return worst


@pytest.mark.parametrize("B", [1, 2])
def test_route_equivalence_tiny(B):
    """Quantised model vs a plain bf16 LMModel holding the dequantised values: the same function in a different summation order, 13
    steps so that the 10-slot ring wraps; rel_err < 1e-3 is the project's model-level tolerance."""
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
    model.quantize_weights_("mxfp4")
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
            assert ("gemv_mxfp4w" in [r[0] for r in recs]) == (B <= 2)
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
    depth phase as persistent launch and as chain."""
    monkeypatch.setenv("NO_CUDA_GRAPH", "0" if graphs else "1")
    monkeypatch.setenv("RST_DEPTH_FRAME", "1" if depth_frame else "0")
    cfg, sd, model = _tiny()
    model.quantize_weights_("mxfp4")
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


def test_eager_frame_profile_shows_every_covered_gemv_quantised(monkeypatch):
    monkeypatch.setenv("NO_CUDA_GRAPH", "1")
    cfg, sd, model = _tiny()
    model.quantize_weights_("mxfp4")
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
    E, Hd, Ed = cfg["dim"], 704, cfg["depformer_dim"]
    want4 = sorted([(1, 3 * E, E), (1, E, E), (1, 2 * Hd, E), (1, E, Hd)] * cfg["num_layers"])
    want8 = sorted([(1, cfg["text_card"], E), (1, cfg["dep_q"] * Ed, E)])
    assert sorted(r[5] for r in recs if r[0] == "gemv_mxfp4w") == want4
    assert sorted(r[5] for r in recs if r[0] == "gemv_fp8w") == want8
    covered = {(n, k) for _, n, k in want4 + want8}
    assert not [r for r in recs if r[0] == "gemv_bf16" and (r[5][1], r[5][2]) in covered]
    for r in recs:
        if r[0] == "gemv_mxfp4w":
            _, N, K = r[5]
            assert r[4] == N * K // 2 + N * K // 32 + 4 * (K + (N // 2 if N == 2 * Hd else N))


def test_no_persistent_temporal_launch_for_a_quantised_model():
    """Past 2048 ring steps a bf16 batch-1 session moves to the persistent temporal launch (and re-captures its frame); an mxfp4 one
    must not: that launch reads the bf16 weights."""
    cfg = dict(synth.LM_MOSHI_7B, num_layers=1)
    model = LMModel.from_state_dict(synth.lm_state_dict(cfg, seed=4, device=DEV), cfg)
    model.quantize_weights_("mxfp4")
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
        names = [r[0] for r in recs]
        assert names.count("gemv_mxfp4w") == 4 and names.count("gemv_fp8w") == 1 and not [n for n in names if n in ("gemv_bf16", "temporal_frame")]


def test_streaming_pipeline_with_an_mxfp4_lm_matches_composed_oracles():
    B, frames = 2, 6
    cfg = dict(synth.LM_TINY_16Q)
    mimi_sd = synth.mimi_state_dict(0)
    lm_sd = synth.lm_state_dict(cfg, seed=9)
    mimi = MimiCodec.from_state_dict(mimi_sd).to(DEV)
    model = LMModel.from_state_dict({k: v.to(DEV) for k, v in lm_sd.items()}, cfg, weight_dtype="mxfp4")
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
