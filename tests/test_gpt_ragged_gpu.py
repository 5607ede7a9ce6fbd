"""Per-stream ring positions on the GPU: the ring kernels of the GPT global transformer with one position per stream (csrc/lm_attn.hip,
csrc/lm_prefill.hip), per-row id limits of the samplers (csrc/lm_sample.hip, csrc/lm_depth.hip), and on top of them ragged
``GPT.forward_global(lengths=)``, per-stream ``GPTGen`` sessions and ``InferenceImp.generate_batch``.

Kernel level: a stream at position p must get EXACTLY what the shared-position launch of the same rows gives at p -- outputs and ring
bytes are compared with ``torch.equal`` against launches of today's entry points, one per distinct position.
Model level: the oracle (oracle/gpt_oracle.py) at the 1e-3 of tests/test_gpt_gpu.py; ``GPTGen`` rings hold context + 1 slots, whose
single steps see the plain context mask (lm/generate.py), so a stream at position p is compared with the oracle's NON-streaming pass
over that stream's own history, last position.  bf16 rings are held to the bound tests/test_gpt_prefill_gpu.py holds them to: 1e-3
against the product's own single-stream pass on bf16 rings (the project has no bf16-ring bound against the fp32 oracle; printed only).
Batched generation must reproduce the oracle's tokens exactly; tests/test_gpt_ragged_cpu.py holds the oracle's decision margins on
these prompts at >= 1e-4, a hundred times the ~1e-6 summation-order noise test_gpt_gpu.py quotes."""
import functools

import pytest
import torch

from oracle import gpt_oracle as Gp
from rstnet_amd import ops
from rstnet_amd.lm.generate import GenIds, GPTGen, InferenceImp
from rstnet_amd.lm.gpt import GPT, Config
from rstnet_amd import synth
from tests.golden import cases
from tests.helpers import gpt_ragged as R
from tests.helpers import lora_bank as LB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3
F32, BF16 = torch.float32, torch.bfloat16
BASE = 10000.0
H, D = 4, 64


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def build(name, overrides=None, **kw):
    cfg_d = dict(R.CFGS[name])
    cfg_d.update(overrides or {})
    sd = {k: v.to(DEV) for k, v in synth.gpt_state_dict(cfg_d, cases.GPT_SEED).items()}
    model = GPT.from_state_dict(sd, Config.from_dict(cfg_d), **kw)
    osd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    return model, R.oracle_config(cfg_d), osd, cfg_d


def _tokens(cfg_d, B, steps, seed):
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(0, cfg_d["padded_vocab_size"], (B, 1, steps), generator=g)
    audio = torch.randint(0, cfg_d["audio_card"] + 1, (B, cfg_d["n_q"], steps), generator=g)
    return torch.cat([text, audio], 1)


# ---------------------------------------------------------------------------------------------------------------- 1 - 3: kernels
def _positions(cap):
    return [0, 1, cap - 1, cap, 3 * cap + 5]


def _rings(B, G, cap, kv, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, G, cap, D, generator=g).to(DEV, kv), torch.randn(B, G, cap, D, generator=g).to(DEV, kv)


@pytest.mark.parametrize("cap,kv,table", [(11, F32, False), (130, F32, False), (130, F32, True), (130, BF16, False), (130, BF16, True)])
@pytest.mark.parametrize("G", [2, 4])
def test_decode_at_per_stream_positions_is_the_shared_position_launch(cap, kv, table, G):
    pos = _positions(cap)
    B = len(pos)
    k0, v0 = _rings(B, G, cap, kv, 1)
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, (H + 2 * G) * D, generator=g).to(DEV)
    kw = dict(rope=True, context=cap - 1, max_period=BASE, heads=H, rope_dims=32, splits=1 if cap <= 64 else 2)
    rot = dict(max_period=BASE, rope_dims=32)

    def run(p):
        k, v = k0.clone(), v0.clone()
        pd = torch.tensor(p, device=DEV, dtype=torch.long)
        tab = ops.lm_rope_table(pd, D, **rot) if table else None
        return ops.lm_attn_decode(qkv, k, v, pd, rope_table=tab, **kw), k, v, tab

    out, k, v, tab = run(pos)
    assert tab is None or tuple(tab.shape) == (B, D // 2, 2)
    for p in sorted(set(pos)):
        out_p, k_p, v_p, tab_p = run([p])
        for b in [b for b in range(B) if pos[b] == p]:
            assert torch.equal(out[b], out_p[b]), (p, b)
            assert torch.equal(k[b], k_p[b]) and torch.equal(v[b], v_p[b]), (p, b)
            assert tab is None or torch.equal(tab[b], tab_p), (p, b)
    assert not torch.equal(k, k0)


@pytest.mark.parametrize("cap,kv", [(11, F32), (130, F32), (130, BF16)])
@pytest.mark.parametrize("Tc", [6, "cap"])
@pytest.mark.parametrize("G", [2, 4])
def test_prefill_and_ragged_append_at_per_stream_positions(cap, kv, Tc, G):
    Tc = cap if Tc == "cap" else Tc
    pos, lens = _positions(cap), [0, 1, Tc - 1, Tc, Tc]
    B = len(pos)
    k0, v0 = _rings(B, G, cap, kv, 3)
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(B, Tc, (H + 2 * G) * D, generator=g).to(DEV)
    freqs = ops.gpt_rope_freqs(torch.device(DEV), BASE, 32)
    kw = dict(rope=True, max_period=BASE, rope_dims=32, heads=H, freqs=freqs)

    def run(p, lengths):
        k, v = k0.clone(), v0.clone()
        pd = torch.tensor(p, device=DEV, dtype=torch.long)
        out = ops.lm_attn_prefill(qkv, k, v, pd, window=cap - 1, **kw)
        assert torch.equal(k, k0) and torch.equal(v, v0)          # the attention appends nothing
        if lengths is None:
            ops.lm_ring_append(qkv, k, v, pd, **kw)
        else:
            ops.lm_ring_append_ragged(qkv, k, v, pd, lengths=lengths, **kw)
        return out.view(B, Tc, -1), k, v

    out, k, v = run(pos, torch.tensor(lens, device=DEV, dtype=torch.int32))
    for p in sorted(set(pos)):
        out_p, k_p, v_p = run([p], None)
        for b in [b for b in range(B) if pos[b] == p]:
            n = lens[b]
            assert torch.equal(out[b, :n], out_p[b, :n]), (p, b)
            new = torch.zeros(cap, dtype=torch.bool)
            new[[(p + t) % cap for t in range(n)]] = True
            for got, ref, old in ((k, k_p, k0), (v, v_p, v0)):
                assert torch.equal(got[b][:, new], ref[b][:, new]), (p, b)
                assert torch.equal(got[b][:, ~new], old[b][:, ~new]), (p, b)      # rows t >= len: slots exactly as before the call
    assert torch.equal(k[0], k0[0]) and torch.equal(v[0], v0[0])                  # a length of 0 takes nothing
    # the chunk offset: lengths count from the start of a call, this chunk being its rows [t0, t0 + Tc)
    k2, v2 = k0.clone(), v0.clone()
    pd = torch.tensor(pos, device=DEV, dtype=torch.long)
    ops.lm_ring_append_ragged(qkv, k2, v2, pd, lengths=torch.tensor([n + 3 for n in lens], device=DEV, dtype=torch.int32), t0=3, **kw)
    assert torch.equal(k2, k) and torch.equal(v2, v)
    k3 = k0.clone()
    ops.lm_ring_append_ragged(qkv, k3, v0.clone(), pd, lengths=torch.tensor([2] * B, device=DEV, dtype=torch.int32), t0=3, **kw)
    assert torch.equal(k3, k0)                                                     # lengths below the offset: nothing


@pytest.mark.parametrize("V,limits", [(320, [300, 40, 320, 100, 26]), (151936, [151936, 30, 40000, 151000, 26])])
def test_sampler_with_one_limit_per_row(V, limits):
    B, k = len(limits), 25
    g = torch.Generator().manual_seed(V)
    # a ramp over the ids puts the unrestricted top-k at the highest ids: every limit below V changes the row's candidates
    logits = (torch.randn(B, V, generator=g) + torch.linspace(0, 8, V)).to(DEV)
    noise = (-torch.log(torch.rand(B, k, generator=g).clamp_min(1e-9))).to(DEV)
    lim = torch.tensor(limits, device=DEV, dtype=torch.int32)
    kw = dict(use_sampling=True, temp=0.8, top_k=k)
    got = ops.lm_sample(logits, noise=noise, limit_dev=lim, **kw)
    # the same batch with every row on the scalar limit of row b: today's entry point, row b of its result
    want = torch.stack([ops.lm_sample(logits, noise=noise, limit_dev=lim[b:b + 1].clone(), **kw)[b] for b in range(B)])
    assert torch.equal(got, want) and bool((got < lim).all())
    alone = torch.cat([ops.lm_sample(logits[b:b + 1], noise=noise[b:b + 1], limit_dev=lim[b:b + 1].clone(), **kw) for b in range(B)])
    assert torch.equal(got, alone)
    uniform = ops.lm_sample(logits, noise=noise, limit_dev=lim[:1].clone(), **kw)
    assert not torch.equal(got, uniform)                                            # the limits matter
    table = torch.stack([lim, lim.flip(0), lim], 1).contiguous()                    # a column of a [B, 3] table: element stride 3
    assert torch.equal(ops.lm_sample(logits, noise=noise, limit_dev=table[:, 1], **kw),
                       ops.lm_sample(logits, noise=noise, limit_dev=lim.flip(0).contiguous(), **kw))
    if V > 32768:       # the one-level kernel of large vocabularies
        assert torch.equal(ops.lm_sample(logits, noise=noise, limit_dev=lim, two_level=False, **kw), got)


@pytest.mark.parametrize("B,persistent", [(2, True), (2, False), (5, False)])
def test_depth_frame_with_one_row_of_limits_per_stream(B, persistent):
    model, ocfg, osd, cfg_d = build("gqa")
    dec, dep, Q, k = model.depth_decoder, model.codecformer, cfg_d["dep_q"], 8
    if persistent:
        Hd = dep.layers[0].gating[0].linear_out.weight.shape[1]
        assert ops.depth_frame_enabled(torch.device(DEV)) and ops.depth_frame_supported(B, dep.d_model, dep.num_heads, Hd, cfg_d["audio_card"], Q,
                                                                                       len(dep.layers), k, device=torch.device(DEV))
    g = torch.Generator().manual_seed(B)
    h = torch.randn(B, cfg_d["n_embd"], generator=g).to(DEV)
    text = torch.randint(0, 300, (B,), generator=g).to(DEV)
    noise = (-torch.log(torch.rand(B, Q * k, generator=g).clamp_min(1e-9))).to(DEV)
    limits = torch.tensor([[31, 30, 9], [10, 31, 30], [30, 12, 31], [8, 8, 8], [31, 31, 31]][:B], device=DEV, dtype=torch.int32)
    pos = torch.arange(Q, device=DEV, dtype=torch.long)
    rings = lambda n: dep._init_streaming_state(n, capacity=Q + 1)

    def run(lim):
        tokens = torch.zeros(B, Q + 1, device=DEV, dtype=torch.long)
        tokens[:, 0] = text
        dec.decode_frame(tokens, h, noise, pos, use_sampling=True, temp=0.8, top_k=k, limits=lim, rings=rings(B), persistent=persistent)
        return tokens[:, 1:].clone()

    got = run(limits)
    for b in range(B):
        assert torch.equal(got[b], run(limits[b].clone())[b]), b
    assert bool((got < limits).all())


# ---------------------------------------------------------------------------------------------------- 4 - 7: forward_global, sessions
RAGGED = [1, 4, 11, 12, 17]      # context 10, ring of 11: one position, inside the ring, exactly full, one past, wrapped


def _oracle_last(osd, ocfg, hist):
    """(h, logits) of the last position of one stream's history ``[1, K, n]``: the oracle's non-streaming pass (plain context mask)."""
    with torch.no_grad():
        h, lg = Gp.forward_global(osd, ocfg, hist, merged=True)
    return h[0, -1], lg[0, -1]


@functools.lru_cache(maxsize=None)
def _oracle_full(name, seed, lengths):
    """Per stream, the oracle's (h, logits) over its own length -- computed once, shared, never modified."""
    model, ocfg, osd, cfg_d = build(name)
    toks = _tokens(cfg_d, len(lengths), max(lengths), seed)
    with torch.no_grad():
        return [Gp.forward_global(osd, ocfg, toks[b:b + 1, :, :n], merged=True) for b, n in enumerate(lengths)]


@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_ragged_forward_global_against_the_oracle_per_stream(name):
    model, ocfg, osd, cfg_d = build(name)
    B, T = len(RAGGED), max(RAGGED)
    toks = _tokens(cfg_d, B, T, 61)
    ref = _oracle_full(name, 61, tuple(RAGGED))
    gen = GPTGen(model, use_sampling=False)
    gen.begin(B, per_stream=True)
    try:
        st = model.transformer._streaming_state
        assert st.k[0].shape[2] == 11 and tuple(st.pos.shape) == (B,)
        h, lg = model.forward_global(toks.to(DEV), RAGGED)
        assert st.pos.tolist() == RAGGED
    finally:
        gen.end()
    h2, lg2 = model.forward_global(toks.to(DEV), torch.tensor(RAGGED))      # outside a session: a temporary per-stream state
    for b, n in enumerate(RAGGED):
        e = (rel_err(h[b, :n], ref[b][0][0]), rel_err(lg[b, :n], ref[b][1][0]), rel_err(h2[b, :n], ref[b][0][0]), rel_err(lg2[b, :n], ref[b][1][0]))
        print(f"{name} ragged forward_global stream {b} len {n}: session h {e[0]:.3e} logits {e[1]:.3e}; outside h {e[2]:.3e} logits {e[3]:.3e}")
        assert max(e) < TOL, (b, e)
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(lg).all())      # rows past a length: unspecified, never NaN from a table


LONG = dict(context=100, block_size=256)
RAGGED_LONG = [2, 65, 100, 101, 140]


@pytest.mark.parametrize("kv", [F32, BF16])
def test_ragged_forward_global_on_long_rings(kv):
    model, ocfg, osd, cfg_d = build("gqa", LONG, kv_dtype=kv)
    B, T = len(RAGGED_LONG), max(RAGGED_LONG)
    toks = _tokens(cfg_d, B, T, 62)
    gen = GPTGen(model, use_sampling=False)
    gen.begin(B, per_stream=True)
    try:
        assert model.transformer._streaming_state.k[0].shape[2] == 101 and model.transformer._streaming_state.k[0].dtype == kv
        h, lg = model.forward_global(toks.to(DEV), RAGGED_LONG)
        steps = _tokens(cfg_d, B, 2, 65)      # two decode steps on the long ring: the per-stream rope table
        after = [model.forward_global(steps[:, :, s:s + 1].to(DEV)) for s in range(2)]
        after = [(a[0][:, 0].clone(), a[1][:, 0].clone()) for a in after]
    finally:
        gen.end()
    for b, n in enumerate(RAGGED_LONG):
        with torch.no_grad():
            h_o, lg_o = Gp.forward_global(osd, ocfg, toks[b:b + 1, :, :n], merged=True)
        e_o = (rel_err(h[b, :n], h_o[0]), rel_err(lg[b, :n], lg_o[0]))
        if kv == F32:
            print(f"fp32 rings of 101, stream {b} len {n}: vs oracle h {e_o[0]:.3e} logits {e_o[1]:.3e}")
            assert max(e_o) < TOL, (b, e_o)
            for s in range(2):
                h_s, lg_s = _oracle_last(osd, ocfg, torch.cat([toks[b:b + 1, :, :n], steps[b:b + 1, :, :s + 1]], 2))
                assert max(rel_err(after[s][0][b], h_s), rel_err(after[s][1][b], lg_s)) < TOL, (b, s)
            continue
        gen.begin(1)          # the same stream alone on bf16 rings of a scalar-position session
        try:
            h1, lg1 = model.forward_global(toks[b:b + 1, :, :n].to(DEV))
        finally:
            gen.end()
        e = (rel_err(h[b, :n], h1[0]), rel_err(lg[b, :n], lg1[0]))
        print(f"bf16 rings of 101, stream {b} len {n}: vs the stream alone h {e[0]:.3e} logits {e[1]:.3e}; vs fp32 oracle h {e_o[0]:.3e} "
              f"logits {e_o[1]:.3e} (printed only)")
        assert max(e) < 1e-3, (b, e)


def _frame_col(toks, t):
    return toks[:, :, t:t + 1]


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_steps_after_a_ragged_prefill(name, graphs, monkeypatch):
    monkeypatch.setenv("NO_CUDA_GRAPH", "0" if graphs else "1")
    model, ocfg, osd, cfg_d = build(name)
    B, T, S = len(RAGGED), max(RAGGED), 12
    toks, steps = _tokens(cfg_d, B, T, 61), _tokens(cfg_d, B, S, 63)
    gen = GPTGen(model, use_sampling=False)
    gen.begin(B, per_stream=True)
    got = []
    try:
        gen.prefill(toks.to(DEV), RAGGED)
        for s in range(S):
            h, lg = model.forward_global(_frame_col(steps, s).to(DEV))
            got.append((h[:, 0].clone(), lg[:, 0].clone()))
        assert model.transformer._streaming_state.pos.tolist() == [n + S for n in RAGGED]
    finally:
        gen.end()
    worst = 0.0
    for b, n in enumerate(RAGGED):
        for s in range(S):
            h_o, lg_o = _oracle_last(osd, ocfg, torch.cat([toks[b:b + 1, :, :n], steps[b:b + 1, :, :s + 1]], 2))
            e = max(rel_err(got[s][0][b], h_o), rel_err(got[s][1][b], lg_o))
            worst = max(worst, e)
            assert e < TOL, (b, s, e)
    print(f"{name} graphs={graphs}: 12 steps after the ragged prefill, worst error vs the oracle {worst:.3e}")


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_a_stream_does_not_depend_on_its_neighbours(name, fp8):
    """Stream 0 -- its prefill rows and 4 following steps -- has the same BITS whatever tokens and lengths its four neighbours have, on the
    default route and on the fp8 route of ``GPT.use_fp8`` (activations are quantised with one scale per row)."""
    model, ocfg, osd, cfg_d = build(name)
    model.use_fp8(fp8)
    B, T, S = len(RAGGED), max(RAGGED), 4
    n0 = 7

    def run(seed, lengths):
        toks, steps = _tokens(cfg_d, B, T, seed), _tokens(cfg_d, B, S, seed + 1)
        toks[0], steps[0] = _tokens(cfg_d, 1, T, 70)[0], _tokens(cfg_d, 1, S, 71)[0]      # stream 0 is the same in both runs
        gen = GPTGen(model, use_sampling=False)
        gen.begin(B, per_stream=True)
        try:
            h, lg = model.forward_global(toks.to(DEV), lengths)
            out = [h[0, :n0].clone(), lg[0, :n0].clone()]
            for s in range(S):
                h, lg = model.forward_global(_frame_col(steps, s).to(DEV))
                out += [h[0].clone(), lg[0].clone()]
        finally:
            gen.end()
        return out

    a, b = run(64, [n0, 4, 11, 12, 17]), run(66, [n0, 17, 1, 0, 9])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_admission_into_a_live_session(name):
    model, ocfg, osd, cfg_d = build(name)
    B, T = len(RAGGED), max(RAGGED)
    toks, step = _tokens(cfg_d, B, T, 61), _tokens(cfg_d, B, 1, 67)
    new_len = 13
    fresh = torch.zeros(B, toks.shape[1], new_len, dtype=torch.long)
    fresh[2] = _tokens(cfg_d, 1, new_len, 68)[0]

    def run(admit):
        gen = GPTGen(model, use_sampling=False)
        gen.begin(B, per_stream=True)
        try:
            gen.prefill(toks.to(DEV), RAGGED)
            row2 = None
            if admit:
                before = [k.clone() for k in model.transformer._streaming_state.k]
                gen.reset_streams([2])
                row2 = gen.prefill(fresh.to(DEV), [0, 0, new_len, 0, 0])
                assert model.transformer._streaming_state.pos.tolist() == [1, 4, new_len, 12, 17]
                for old, now in zip(before, model.transformer._streaming_state.k):
                    assert torch.equal(old[[0, 1, 3, 4]], now[[0, 1, 3, 4]])
            h, lg = model.forward_global(step.to(DEV))
            return row2, h[:, 0].clone(), lg[:, 0].clone()
        finally:
            gen.end()

    _, h_a, lg_a = run(False)
    row2, h_b, lg_b = run(True)
    h_o, lg_o = _oracle_last(osd, ocfg, fresh[2:3])
    e = (rel_err(row2[0][2], h_o), rel_err(row2[1][2], lg_o))
    print(f"{name} admission: the new prompt in row 2 vs the oracle on a fresh state h {e[0]:.3e} logits {e[1]:.3e}")
    assert max(e) < TOL
    others = [0, 1, 3, 4]
    assert torch.equal(h_a[others], h_b[others]) and torch.equal(lg_a[others], lg_b[others])
    h_o, lg_o = _oracle_last(osd, ocfg, torch.cat([fresh[2:3], step[2:3]], 2))
    assert max(rel_err(h_b[2], h_o), rel_err(lg_b[2], lg_o)) < TOL


# ------------------------------------------------------------------------------------------------------------ 8: batched generation
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_generate_batch_reproduces_the_oracle_per_prompt(name, sampled):
    model, ocfg, osd, cfg_d = build(name)
    seqs = R.prompts(cfg_d)
    ref, margin = R.oracle_generate(osd, ocfg, cfg_d, sampled)
    assert margin >= R.MARGIN          # (the weights merged on the device are the ones the CPU test measured, to rounding of the merge)
    ids = GenIds(text_initial_token_id=R.TEXT_INIT, **R.IDS)
    s = R.SAMPLING
    imp = InferenceImp(None, model, "sample", s["temp_text"], s["top_k_text"], s["temp"], s["top_k"], "TTS", use_sampling=sampled, ids=ids,
                       noise=R.batch_noise(len(seqs)))
    outs = imp.generate_batch(seqs)
    assert len(outs) == len(seqs) and len({o["frames"].shape[0] for o in outs}) > 1
    for b, (out, want) in enumerate(zip(outs, ref)):
        assert torch.equal(out["frames"].cpu(), want["frames"]), b
        assert torch.equal(out["text"].cpu(), want["text"]), b
    if not sampled:      # the production configuration: captured graphs, no noise hook
        imp_g = InferenceImp(None, model, "sample", s["temp_text"], s["top_k_text"], s["temp"], s["top_k"], "TTS", use_sampling=False, ids=ids)
        for out, want in zip(imp_g.generate_batch(seqs), ref):
            assert torch.equal(out["frames"].cpu(), want["frames"]) and torch.equal(out["text"].cpu(), want["text"])


# --------------------------------------------------------------------------------------------------------- 9: adapter bank, ragged
def test_adapter_bank_with_ragged_lengths():
    cfg_d = LB.CFGS["gqa"]
    base = {k: v.to(DEV) for k, v in LB.base_sd(cfg_d).items()}
    sets = [{k: v.to(DEV) for k, v in s.items()} for s in LB.adapter_sets(cfg_d)][:2]
    model = GPT.from_state_dict({k: v.clone() for k, v in base.items()}, Config.from_dict(cfg_d), merge_lora=False)
    model.load_adapter_bank(sets)
    ids = [0, 1, -1, 0, 1]
    B, T = len(RAGGED), max(RAGGED)
    toks = _tokens(cfg_d, B, T, 69)
    gen = GPTGen(model, use_sampling=False)
    gen.begin(B, adapter_ids=ids, per_stream=True)
    try:
        h, lg = model.forward_global(toks.to(DEV), RAGGED)
    finally:
        gen.end()
    keep = set(Gp.GPTConfig.__dataclass_fields__)
    for b, (n, k) in enumerate(zip(RAGGED, ids)):
        ocfg = Gp.GPTConfig(**{a: v for a, v in {**cfg_d, **({"lora_r": 0} if k < 0 else {})}.items() if a in keep})
        osd = {a: v.float().cpu() for a, v in {**base, **({} if k < 0 else sets[k])}.items()}
        with torch.no_grad():
            h_o, lg_o = Gp.forward_global(osd, ocfg, toks[b:b + 1, :, :n])
        e = (rel_err(h[b, :n], h_o[0]), rel_err(lg[b, :n], lg_o[0]))
        assert max(e) < TOL, (b, k, e)
