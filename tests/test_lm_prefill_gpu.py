"""Multi-position (prefill) pass of the Moshi-style LM: the attention kernel and the ring append against an fp64 evaluation of the
window definition, ``LMModel.forward_text`` with S > 1 against the stepped oracle, ``forward`` / ``forward_local`` against the imported
reference (fixture ``lm_tiny_forward.npz``), and ``LMGen.prefill`` against the reference's own token streams (``lm_tiny.npz``).

Tolerances are the ones the repository applies to the same quantities against the same oracles: attention 1e-4 (fp32 rings) / 3e-3
(bf16 rings) and ring keys 1e-4 / 1e-2 with bit-identical values (``_ring_attention_case`` of test_lm_gpu.py), logits and hidden
states 1e-3, greedy tokens exact."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import lm_oracle as L
from rstnet_amd import ops, synth
from rstnet_amd.lm.model import LMGen, LMModel
from tests.golden import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_PERIOD = 10000.0


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _rope(x: torch.Tensor, pos0: int, dtype=torch.float32) -> torch.Tensor:
    """apply_rope (modules/rope.py:11-68) on x [B,H,T,D] at positions pos0 .. pos0 + T - 1: the angle is the reference's fp32 product
    (that IS the definition); ``dtype=float64`` evaluates cos / sin and the rotation itself in fp64."""
    D, T = x.shape[-1], x.shape[-2]
    ds = torch.arange(D // 2, dtype=torch.float32)
    freqs = torch.exp(ds * (-math.log(MAX_PERIOD) * 2 / D))
    ang = (freqs * (torch.tensor([pos0]).float() + torch.arange(T, dtype=torch.float32)).view(-1, 1)).to(dtype)
    xr, xi = x.to(dtype).reshape(*x.shape[:-1], D // 2, 2).unbind(-1)
    return torch.stack([xr * torch.cos(ang) - xi * torch.sin(ang), xr * torch.sin(ang) + xi * torch.cos(ang)], -1).reshape(x.shape)


def _chunks(H, cap, T):
    if T <= cap:
        return [T]
    out, sizes, i = [], [3, 4, 7, min(cap, 10), 1], 0          # chunk boundaries that straddle the wrap of a short ring
    while sum(out) < T:
        out.append(min(sizes[i % len(sizes)], cap, T - sum(out)))
        i += 1
    return out


PREFILL_CASES = [(2, 64, 10, 10, 0, 25), (4, 64, 300, 250, 280, 70), (32, 128, 300, 300, 0, 130), (8, 128, 3000, 3000, 2990, 40),
                 (32, 128, 3000, 3000, 2900, 256)]
# fp32 rings everywhere; bf16 rings where the model allows them (rings of <= 64 slots are always fp32: _init_streaming_state)
PREFILL_PARAMS = [c + (dt,) for c in PREFILL_CASES for dt in (torch.float32, torch.bfloat16) if dt == torch.float32 or c[2] > 64]


@pytest.mark.parametrize("H,D,cap,context,start,T,kv_dtype", PREFILL_PARAMS)
def test_prefill_attention_and_append_against_fp64(H, D, cap, context, start, T, kv_dtype):
    """`ops.lm_attn_prefill` + `ops.lm_ring_append`, chunk by chunk, on an empty / partly filled / wrapped ring.  Reference: softmax over
    the keys max(0, p - W + 1) .. p, W = min(context, cap - 1), in fp64 over the values the ring stores (read back after the append:
    the bytes a later step reads); the rings themselves against an oracle ring (fp32 rotation, rounded to the ring's dtype); and the same
    chunk fed as single `ops.lm_attn_decode` steps on cloned rings."""
    B = 2
    bound = 1e-4 if kv_dtype == torch.float32 else 3e-3
    W = min(context, cap - 1)
    g = torch.Generator().manual_seed(H * D + start)
    # a ring as `start` single steps would have left it: position p in slot p % cap
    n_old = min(start, cap)
    k_ref, v_ref = torch.zeros(B, H, cap, D), torch.zeros(B, H, cap, D)           # the oracle ring (fp32 numbers representable in kv_dtype)
    P = start + T
    kpos = torch.zeros(B, H, P, D, dtype=torch.float64)                            # stored values by POSITION (what the fp64 reference reads)
    vpos = torch.zeros(B, H, P, D, dtype=torch.float64)
    if n_old:
        old = torch.arange(start - n_old, start)
        k_ref[:, :, old % cap] = (0.5 * torch.randn(B, H, n_old, D, generator=g)).to(kv_dtype).float()
        v_ref[:, :, old % cap] = (0.5 * torch.randn(B, H, n_old, D, generator=g)).to(kv_dtype).float()
        kpos[:, :, old], vpos[:, :, old] = k_ref[:, :, old % cap].double(), v_ref[:, :, old % cap].double()
    kc, vc = k_ref.to(DEV, kv_dtype), v_ref.to(DEV, kv_dtype)
    pos = torch.full((1,), start, dtype=torch.long, device=DEV)
    p0, worst, worst_steps = start, 0.0, 0.0
    for Tc in _chunks(H, cap, T):
        qkv = torch.randn(B, Tc, 3 * H * D, generator=g)
        q, k, v = qkv.view(B, Tc, 3, H, D).permute(2, 0, 3, 1, 4)                  # [B,H,Tc,D]
        qd = qkv.to(DEV)
        k2, v2 = kc.clone(), vc.clone()
        out = ops.lm_attn_prefill(qd, kc, vc, pos, window=W, rope=True, max_period=MAX_PERIOD)
        assert torch.equal(kc, k2) and torch.equal(vc, v2), "the attention launch must not touch the ring"
        ops.lm_ring_append(qd, kc, vc, pos, rope=True, max_period=MAX_PERIOD)
        # oracle ring
        new = torch.arange(p0, p0 + Tc)
        k_ref[:, :, new % cap] = _rope(k, p0).to(kv_dtype).float()
        v_ref[:, :, new % cap] = v.to(kv_dtype).float()
        kpos[:, :, new], vpos[:, :, new] = kc[:, :, (new % cap).to(DEV)].double().cpu(), vc[:, :, (new % cap).to(DEV)].double().cpu()
        # fp64 reference of the window definition (on the device: torch's fp64 matmul, none of this library's kernels)
        lo = max(0, p0 - W + 1)
        q64 = _rope(q, p0, torch.float64).to(DEV)
        kk, vv = kpos[:, :, lo:p0 + Tc].to(DEV), vpos[:, :, lo:p0 + Tc].to(DEV)
        pq, pk = torch.arange(p0, p0 + Tc, device=DEV).view(-1, 1), torch.arange(lo, p0 + Tc, device=DEV).view(1, -1)
        mask = (pk <= pq) & (pk >= pq - W + 1)
        sc = (q64 @ kk.transpose(-1, -2)) / math.sqrt(D)
        ref = torch.softmax(sc.masked_fill(~mask, float("-inf")), -1) @ vv            # [B,H,Tc,D]
        ref = ref.permute(0, 2, 1, 3).reshape(B * Tc, H * D)
        e = rel_err(out, ref)
        worst = max(worst, e)
        print(f"prefill H={H} D={D} cap={cap} ctx={context} pos={p0} Tc={Tc} {kv_dtype}: rel_err {e:.3e}")
        assert e < bound, f"chunk at position {p0}"
        # the same chunk as Tc single decode steps on the cloned rings
        p2 = pos.clone()
        steps = []
        for t in range(Tc):
            steps.append(ops.lm_attn_decode(qd[:, t].contiguous(), k2, v2, p2, rope=True, context=context, max_period=MAX_PERIOD))
            p2.add_(1)
        e2 = rel_err(out.view(B, Tc, H * D), torch.stack(steps, 1))
        worst_steps = max(worst_steps, e2)
        assert e2 < 2 * bound, f"chunk at position {p0} against single steps: {e2:.3e}"
        assert torch.equal(v2, vc), "value rings of the two routes"
        pos.add_(Tc)
        p0 += Tc
    print(f"prefill H={H} D={D} cap={cap}: worst vs fp64 {worst:.3e}, worst vs single steps {worst_steps:.3e}")
    if kv_dtype == torch.float32:
        assert torch.equal(vc.cpu(), v_ref)
        assert rel_err(kc, k_ref) < 1e-4
    else:
        assert torch.equal(vc.float().cpu(), v_ref)
        assert rel_err(kc.float(), k_ref) < 1e-2


def test_prefill_refuses_unserved_shapes():
    H, D, cap = 2, 64, 16
    kc, vc = torch.zeros(1, H, cap, D, device=DEV), torch.zeros(1, H, cap, D, device=DEV)
    pos = torch.zeros(1, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError):        # more new positions than the ring has slots
        ops.lm_attn_prefill(torch.zeros(1, cap + 1, 3 * H * D, device=DEV), kc, vc, pos, window=cap - 1, rope=True)
    with pytest.raises(ValueError):
        ops.lm_ring_append(torch.zeros(1, cap + 1, 3 * H * D, device=DEV), kc, vc, pos, rope=True)
    with pytest.raises(ValueError):        # a window the ring cannot hold
        ops.lm_attn_prefill(torch.zeros(1, 4, 3 * H * D, device=DEV), kc, vc, pos, window=cap + 1, rope=True)
    k32 = torch.zeros(1, H, cap, 32, device=DEV)
    with pytest.raises(ValueError):        # head dim 32
        ops.lm_attn_prefill(torch.zeros(1, 4, 3 * H * 32, device=DEV), k32, k32.clone(), pos, window=4, rope=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lm_attn_prefill(torch.zeros(1, 4, 3 * H * D), kc, vc, pos, window=4, rope=True)


def test_ring_append_without_a_frequency_table(monkeypatch):
    """The C entry points take the frequency table as optional; without it the kernel evaluates exp(i * rope_coef) itself (correctly
    rounded).  At positions up to 21 an ulp of a frequency moves an angle by at most 21 * 6e-8 = 1.3e-6 rad, so both forms sit within the
    fp32 ring bound of 1e-4 of the oracle, and of each other."""
    B, H, D, cap, start, Tc = 1, 2, 64, 16, 14, 8          # wraps inside the chunk
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, Tc, 3 * H * D, generator=g)
    k = qkv.view(B, Tc, 3, H, D).permute(2, 0, 3, 1, 4)[1]
    pos = torch.full((1,), start, dtype=torch.long, device=DEV)
    rings = []
    for table in (True, False):
        if not table:
            monkeypatch.setattr(ops, "_rope_freqs", lambda *a: None)
        kc, vc = torch.zeros(B, H, cap, D, device=DEV), torch.zeros(B, H, cap, D, device=DEV)
        ops.lm_ring_append(qkv.to(DEV), kc, vc, pos, rope=True, max_period=MAX_PERIOD)
        rings.append(kc[:, :, (torch.arange(start, start + Tc) % cap).to(DEV)].cpu())
        assert rel_err(rings[-1], _rope(k, start)) < 1e-4
    assert rel_err(rings[0], rings[1]) < 1e-4


# ---- forward_text with S > 1
def _tiny():
    cfg = dict(synth.LM_TINY)
    sd = synth.lm_state_dict(cfg, cases.LM_SEED)
    model = LMModel.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, cfg)
    return cfg, sd, model


def test_forward_text_chunks_equal_the_stepped_oracle_across_the_wrap():
    """Tiny model inside ``streaming()``: chunks of 3, 4 and 7 positions (the 10-slot ring wraps inside the third) against
    ``lm_oracle.forward_text`` fed one position at a time."""
    cfg, sd, model = _tiny()
    ocfg = L.LMConfig(**cfg)
    sdf = {k: v.float() for k, v in sd.items()}
    B = cases.LM_BATCH
    gt = torch.Generator().manual_seed(15)
    st = L.new_transformer_state(B, ocfg.num_layers, ocfg.num_heads, ocfg.dim // ocfg.num_heads, ocfg.context)
    with model.streaming(B), torch.no_grad():
        for S in (3, 4, 7):
            toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, S), generator=gt)
            toks[0, 2, 0] = -1
            ref = [L.forward_text(sdf, ocfg, toks[:, :, t:t + 1], st) for t in range(S)]
            ref_out, ref_logits = torch.cat([r[0] for r in ref], 1), torch.cat([r[1] for r in ref], 2)
            out, logits = model.forward_text(toks.to(DEV))
            assert out.shape == (B, S, cfg["dim"]) and logits.shape == (B, 1, S, ref_logits.shape[-1])
            e_out, e_log = rel_err(out, ref_out), rel_err(logits, ref_logits)
            print(f"forward_text S={S}: transformer_out {e_out:.3e} logits {e_log:.3e}")
            assert e_out < 1e-3 and e_log < 1e-3, f"chunk of {S}"
        tst = model.transformer._streaming_state
        assert int(tst.pos) == 14 == tst.offset_cpu == st.offset


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("start,S", [(2990, 14), (2900, 200)])
def test_forward_text_chunk_at_the_moshi_shape_across_the_ring_wrap(B, start, S):
    """The two-layer Moshi-7B shape of test_real_shapes_gpu.py (bf16 rings of 3000 slots seeded at ``start``): ONE ``forward_text`` call
    of S positions against the oracle stepped S times; 200 rows are more than three 64-row GEMM chunks."""
    from tests.test_real_shapes_gpu import _seed_rings, _temporal_models
    cfg, model, osd = _temporal_models()
    ocfg = L.LMConfig(**cfg)
    g = torch.Generator().manual_seed(160 + B + S)
    with model.streaming(B), torch.no_grad():
        st_o = L.new_transformer_state(B, cfg["num_layers"], cfg["num_heads"], cfg["dim"] // cfg["num_heads"], cfg["context"])
        _seed_rings(model, st_o, B, start, seed=17 + B)
        toks = torch.randint(0, cfg["card"], (B, cfg["n_q"] + 1, S), generator=g)
        toks[:, 0] = torch.randint(0, cfg["text_card"], (B, S), generator=g)
        out, logits = model.forward_text(toks.to(DEV))
        ref = [L.forward_text(osd, ocfg, toks[:, :, t:t + 1], st_o) for t in range(S)]
        out_o, logits_o = torch.cat([r[0] for r in ref], 1), torch.cat([r[1] for r in ref], 2)
        assert int(model.transformer._streaming_state.pos) == start + S == st_o.offset
    e_out, e_log = rel_err(out, out_o), rel_err(logits, logits_o)
    agree = int((logits.view(B * S, -1).argmax(-1).cpu() == logits_o.reshape(B * S, -1).argmax(-1)).sum())
    print(f"moshi forward_text B={B} start={start} S={S}: transformer_out {e_out:.3e} logits {e_log:.3e} argmax {agree}/{B * S}")
    assert e_out < 1e-3 and e_log < 1e-3
    assert agree == B * S


# ---- forward / forward_local against the imported reference
def test_forward_and_forward_local_match_the_reference_fixture():
    """``LMModel.forward`` is the NON-streaming pass (window = context, no ring quirk): positions 9 .. 13 of the 14 are the ones where a
    pass with the streaming window would be off by 0.17 - 0.37 relative (printed by make_lm_forward_golden.py)."""
    cfg, sd, model = _tiny()
    g = np.load(os.path.join(G, "lm_tiny_forward.npz"))
    seq = torch.from_numpy(g["sequence"]).long().to(DEV)
    audio_logits, text_logits = model.forward(seq)
    assert audio_logits.shape == g["audio_logits"].shape and text_logits.shape == g["text_logits"].shape
    e_a, e_t = rel_err(audio_logits, torch.from_numpy(g["audio_logits"])), rel_err(text_logits, torch.from_numpy(g["text_logits"]))
    late = rel_err(text_logits[:, 9:], torch.from_numpy(g["text_logits"])[:, 9:])
    print(f"forward: audio_logits {e_a:.3e} text_logits {e_t:.3e} (positions 9..13: {late:.3e})")
    assert e_a < 1e-3 and e_t < 1e-3 and late < 1e-3
    assert model.transformer._streaming_state is None and model.depformer._streaming_state is None
    # forward_local on its own, from the reference's transformer_out: int64 start ids and the float embedding of the same ids
    tout = torch.from_numpy(g["transformer_out"]).to(DEV)
    ids, lseq = torch.from_numpy(g["local_ids"]).long().to(DEV), torch.from_numpy(g["local_sequence"]).long().to(DEV)
    ref = torch.from_numpy(g["local_logits"])
    by_ids = model.forward_local(ids, lseq, tout)
    by_emb = model.forward_local(model.depformer_text_emb(ids), lseq, tout)
    print(f"forward_local: ids {rel_err(by_ids, ref):.3e} embedding {rel_err(by_emb, ref):.3e}")
    assert by_ids.shape == ref.shape and rel_err(by_ids, ref) < 1e-3 and rel_err(by_emb, ref) < 1e-3


# ---- LMGen.prefill
def _gold():
    gold = torch.from_numpy(np.load(os.path.join(G, "lm_tiny.npz"))["tokens"]).long()
    return gold                                                      # [B, dep_q + 1, LM_STEPS], -9 where step returned None


def _run_session(gen, cfg, user, plan):
    """plan: list of ("step", n) / ("prefill", n) over consecutive frames; returns the step outputs by frame (None kept)."""
    gold = _gold()
    own = gen.model_time(gold[:, :, gen.max_delay:].to(DEV))          # frames 0 .. LM_STEPS - max_delay - 1
    users = torch.cat(list(user), -1).to(DEV)                        # [B, Ki, LM_STEPS]
    outs, f = {}, 0
    for kind, n in plan:
        if kind == "prefill":
            assert gen.prefill(users[:, :, f:f + n], own[:, :, f:f + n]) is None
            f += n
        else:
            for _ in range(n):
                outs[f] = gen.step(user[f].to(DEV))
                f += 1
    return outs


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("P", [1, 3, 9, 10, 13])
def test_lmgen_prefill_then_steps_equal_the_reference_stream(P, graphs, monkeypatch):
    """Prefill P recorded frames, then step frames P .. 13: the outputs are the fixture's columns P .. 13 exactly."""
    monkeypatch.setenv("NO_CUDA_GRAPH", "0" if graphs else "1")
    cfg, sd, model = _tiny()
    gold, user = _gold(), cases.lm_user_tokens(cfg)
    gen = LMGen(model, use_sampling=False)
    with gen.streaming(cases.LM_BATCH):
        outs = _run_session(gen, cfg, user, [("prefill", P), ("step", cases.LM_STEPS - P)])
        state, tst = gen._streaming_state, model.transformer._streaming_state
        assert state.offset == cases.LM_STEPS == int(state.offset_dev) == int(tst.pos) == tst.offset_cpu and state.temporal_base == 0
    for f in range(P, cases.LM_STEPS):
        assert outs[f] is not None and torch.equal(outs[f][..., 0].cpu(), gold[..., f]), f"frame {f}"


@pytest.mark.parametrize("graphs", [False, True])
def test_lmgen_prefill_in_mid_session(graphs, monkeypatch):
    """4 stepped frames (with graphs: warm-up, capture, replays), 5 prefilled, the rest stepped (the captured frame keeps replaying)."""
    monkeypatch.setenv("NO_CUDA_GRAPH", "0" if graphs else "1")
    cfg, sd, model = _tiny()
    gold, user = _gold(), cases.lm_user_tokens(cfg)
    gen = LMGen(model, use_sampling=False)
    with gen.streaming(cases.LM_BATCH):
        outs = _run_session(gen, cfg, user, [("step", 4), ("prefill", 5), ("step", cases.LM_STEPS - 9)])
    for f in list(range(4)) + list(range(9, cases.LM_STEPS)):
        if f < gen.max_delay:
            assert outs[f] is None
        else:
            assert torch.equal(outs[f][..., 0].cpu(), gold[..., f]), f"frame {f}"


def test_lmgen_prefill_session_state_equals_the_stepped_one():
    """After a prefill the session is indistinguishable from the stepped one: token ring, counters, and the temporal KV rings up to
    the summation-order difference of the two routes."""
    cfg, sd, model = _tiny()
    user = cases.lm_user_tokens(cfg)
    snap = {}
    for route in ("stepped", "prefilled"):
        gen = LMGen(model, use_sampling=False)
        with gen.streaming(cases.LM_BATCH):
            _run_session(gen, cfg, user, [("step", 12)] if route == "stepped" else [("step", 2), ("prefill", 10)])
            state, tst = gen._streaming_state, model.transformer._streaming_state
            snap[route] = (state.cache.clone(), state.offset, int(state.offset_dev), int(tst.pos), tst.offset_cpu, state.temporal_base,
                           [k.clone() for k in tst.k], [v.clone() for v in tst.v])
    a, b = snap["stepped"], snap["prefilled"]
    assert torch.equal(a[0], b[0]) and a[1:6] == b[1:6]
    for ka, kb in zip(a[6] + a[7], b[6] + b[7]):
        assert rel_err(kb, ka) < 1e-3


def test_lmgen_prefill_argument_checks():
    cfg, sd, model = _tiny()
    gen = LMGen(model, use_sampling=False)
    B, Ki, n = 1, cfg["n_q"] - cfg["dep_q"], cfg["dep_q"] + 1
    z = lambda k, t: torch.zeros(B, k, t, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError):
        gen.prefill(z(Ki, 3), z(n, 3))
    with gen.streaming(B):
        with pytest.raises(AssertionError):
            gen.prefill(z(Ki + 1, 3), z(n, 3))
        with pytest.raises(AssertionError):
            gen.prefill(z(Ki, 3), z(n + 1, 3))
        with pytest.raises(AssertionError):
            gen.prefill(z(Ki, 3), z(n, 4))
