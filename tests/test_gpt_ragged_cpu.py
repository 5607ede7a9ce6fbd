"""Host side of per-stream ring positions and ragged batched generation (lm/stack.py, lm/gpt.py, lm/generate.py): the chunk plan of a
per-stream state, the per-stream blanking regimes against the oracle's ``wide`` rule, argument validation, the host bookkeeping of
``InferenceImp.generate_batch`` against a stand-in generator -- and the CONDITION the GPU identity test rests on: the CPU oracle's own
decision margins on the six prompts of tests/helpers/gpt_ragged.py are at least 1e-4 (see that module's docstring)."""
import types

import pytest
import torch

from rstnet_amd import ops, synth
from rstnet_amd.lm import model as lm_model
from rstnet_amd.lm import stack
from rstnet_amd.lm.generate import GenIds, GPTGen, InferenceImp, blanking_regime, regime_wide
from rstnet_amd.lm.gpt import GPT, Config
from tests.helpers import gpt_ragged as R


def _cpu_model(cfg_d, seed=1):
    return GPT.from_state_dict(synth.gpt_state_dict(cfg_d, seed), Config.from_dict(dict(cfg_d)))


# ---- the chunk plan of a per-stream state
def test_per_stream_plan_is_all_prefill_with_chunks_of_the_ring():
    assert stack.per_stream_chunks(11, 17, 256) == [(0, 11, stack.ROUTE_PREFILL), (11, 6, stack.ROUTE_PREFILL)]
    assert stack.per_stream_chunks(101, 140, 256) == [(0, 101, stack.ROUTE_PREFILL), (101, 39, stack.ROUTE_PREFILL)]
    assert stack.per_stream_chunks(3001, 600, 256) == [(0, 256, stack.ROUTE_PREFILL), (256, 256, stack.ROUTE_PREFILL), (512, 88, stack.ROUTE_PREFILL)]
    # a one-position tail stays on the prefill route: the decode kernels know no lengths
    assert stack.per_stream_chunks(11, 12, 256)[-1] == (11, 1, stack.ROUTE_PREFILL)


def test_chunk_advance_is_the_clamp_per_stream():
    lengths = [1, 4, 11, 12, 17]
    plan = stack.per_stream_chunks(11, 17, 256)
    adv = [stack.chunk_advance(lengths, t0, Tc) for t0, Tc, _ in plan]
    assert adv == [[1, 4, 11, 11, 11], [0, 0, 0, 1, 6]]
    assert [sum(a[b] for a in adv) for b in range(5)] == lengths
    assert stack.chunk_advance([0, 3], 0, 2) == [0, 2]


def test_plan_of_the_gpt_transformer_on_either_kind_of_state(monkeypatch):
    model = _cpu_model(synth.GPT_TINY_GQA)
    tr = model.transformer
    shared, per = tr._make_state(3, 11), tr._make_state(3, 11, per_stream=True)
    assert tuple(shared.pos.shape) == (1,) and not shared.per_stream
    assert tuple(per.pos.shape) == (3,) and per.pos.dtype == torch.int64 and per.per_stream
    per.pos += 5
    per.reset()
    assert per.pos.tolist() == [0, 0, 0]
    # scalar-position sessions keep their plans (append-first below the ring's capacity, a decode step for a lone position)
    assert tr.plan(6, shared) == [(0, 6, stack.ROUTE_APPEND_FIRST)]
    assert tr.plan(1, shared) == [(0, 1, stack.ROUTE_DECODE)]
    # per-stream: a lone position without lengths is a decode step; everything else attends before it appends, whatever the mirror says
    assert tr.plan(1, per) == [(0, 1, stack.ROUTE_DECODE)]
    assert tr.plan(1, per, ragged=True) == [(0, 1, stack.ROUTE_PREFILL)]
    per.offset_cpu = 0
    assert tr.plan(6, per) == [(0, 6, stack.ROUTE_PREFILL)]
    assert tr.plan(17, per, ragged=True) == [(0, 11, stack.ROUTE_PREFILL), (11, 6, stack.ROUTE_PREFILL)]
    monkeypatch.setattr(lm_model, "PREFILL_CHUNK", 4)
    assert [c[:2] for c in tr.plan(10, per)] == [(0, 4), (4, 4), (8, 2)]


# ---- blanking regimes
@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_regime_table_is_the_oracles_wide_rule(name):
    """For each of the six prompts and every frame it may generate: the flags ``generate_batch`` writes for the stream's regime are the
    oracle's ``wide = g_len == pre_gen_len or (l_idx > 0 and g_len > minlen)`` (oracle/gpt_generate_oracle.py)."""
    from oracle import gpt_generate_oracle as GG
    cfg_d = dict(R.CFGS[name])
    for seq in R.prompts(cfg_d):
        prefix, maxlen, minlen = GG.split_prompt(seq.unsqueeze(0), "TTS", GG.GenIds(text_initial_token_id=R.TEXT_INIT, **R.IDS))
        pre = prefix.shape[2]
        assert maxlen >= 2
        for g_idx in range(maxlen):
            g_len = pre + g_idx
            want = [g_len == pre or (l > 0 and g_len > minlen) for l in range(cfg_d["dep_q"])]
            assert regime_wide(blanking_regime(pre, minlen, g_idx), cfg_d["dep_q"]) == want, (pre, minlen, g_idx)


# ---- the condition of the GPU identity test: the oracle's own margins
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_oracle_margins_on_the_six_prompts(name, sampled):
    outs, margin = R.cpu_oracle_runs(name, sampled)
    n = [o["frames"].shape[0] for o in outs]
    print(f"{name} sampled={sampled}: frames per prompt {n}, smallest decision margin {margin:.3e}")
    assert all(k >= 1 for k in n) and len(set(n)) > 1          # streams finish at different frames
    assert margin >= R.MARGIN


# ---- argument validation (all raised on the host, before any launch)
def test_lengths_out_of_range_are_refused():
    model = _cpu_model(synth.GPT_TINY_GQA)
    toks = torch.zeros(2, model.num_codebooks, 4, dtype=torch.long)
    for bad in ([1, 5], [-1, 2], [1], [1, 2, 3]):
        with pytest.raises(ValueError, match="lengths must be"):
            model.forward_global(toks, bad)
    with pytest.raises(ValueError, match="lengths must be"):
        model.forward_global(toks, torch.tensor([1, 9]))


def test_lengths_need_a_per_stream_session():
    model = _cpu_model(synth.GPT_TINY_GQA)
    toks = torch.zeros(2, model.num_codebooks, 4, dtype=torch.long)
    with model.streaming(2):
        with pytest.raises(ValueError, match="per-stream"):
            model.forward_global(toks, [1, 2])
    gen = GPTGen(model, use_sampling=False)
    gen.begin(2)
    try:
        with pytest.raises(ValueError, match="per-stream"):
            gen.prefill(toks, [1, 2])
        with pytest.raises(ValueError, match="per-stream"):
            gen.reset_streams([0])
        # a scalar-position session keeps its [dep_q] limits for [dep_q] flags, and moves to a table when it is handed one
        gen.set_blanking([False, True, True])
        assert gen._limits.tolist() == [2048, 2049, 2049]
        gen.set_blanking([[True, False, True], [False, False, True]])
        assert gen._limits.tolist() == [[2049, 2048, 2049], [2048, 2048, 2049]]
    finally:
        gen.end()
    gen.begin(2, per_stream=True)
    try:
        assert tuple(gen._limits.shape) == (2, model.config.dep_q)
        with pytest.raises(ValueError, match="outside"):
            gen.reset_streams([2])
        with pytest.raises(ValueError, match="table"):
            gen.set_blanking([[True] * model.config.dep_q])
        gen.set_blanking([[True, False, True], [False, False, True]])
        assert gen._limits.tolist() == [[2049, 2048, 2049], [2048, 2048, 2049]]
        gen.set_blanking([False, True, False])
        assert gen._limits.tolist() == [[2048, 2049, 2048]] * 2
        model.transformer._streaming_state.pos += 7
        gen.reset_streams([1])
        assert model.transformer._streaming_state.pos.tolist() == [7, 0]
    finally:
        gen.end()


def test_head_size_32_is_refused_when_the_session_opens():
    model = _cpu_model(synth.GPT_GEN_TINY)
    assert model.config.head_size == 32
    with pytest.raises(ValueError, match="head size 32"):
        GPTGen(model, use_sampling=False).begin(2, per_stream=True)
    assert model.transformer._streaming_state is None
    toks = torch.zeros(2, model.num_codebooks, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="head size 32"):
        model.forward_global(toks, [1, 2])


@pytest.mark.parametrize("op", ["lm_rope_append", "attention", "gemv_attn", "attention_step", "rope_split", "temporal_decode_frame",
                                "codec_transformer_frame"])
def test_wrappers_outside_the_gpt_ring_refuse_a_position_vector(op):
    with pytest.raises(ValueError, match="one position for all streams"):
        ops._shared_pos(torch.zeros(3, dtype=torch.int64), op)
    ops._shared_pos(torch.zeros(1, dtype=torch.int64), op)
    ops._shared_pos(None, op)
    import inspect
    assert f'_shared_pos(pos_dev, "{op}")' in inspect.getsource(getattr(ops, op))


def test_position_vector_shapes():
    assert ops._pos_stride(torch.zeros(1, dtype=torch.int64), 4, "x") == 0
    assert ops._pos_stride(torch.zeros(4, dtype=torch.int64), 4, "x") == 1
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="one per stream"):
            ops._pos_stride(bad, 4, "x")


# ---- generate_batch: host bookkeeping against a stand-in generator
class _ScriptedGen:
    """Stands in for ``GPTGen``: frame ``g`` of stream ``b`` is ``script[b][g]`` (dep_q ids); records what the loop asks of it."""

    def __init__(self, script, dep_q):
        self.script, self.dep_q, self.log = script, dep_q, []

    def begin(self, B, per_stream=False):
        self.log.append(("begin", B, per_stream))

    def end(self):
        self.log.append(("end",))

    def prefill(self, tokens, lengths):
        self.log.append(("prefill", tuple(tokens.shape), list(lengths)))
        self.tokens = tokens.clone()
        return torch.zeros(tokens.shape[0], 1), torch.zeros(tokens.shape[0], 1)

    def set_blanking(self, wide):
        self.log.append(("blank", [list(r) for r in wide]))

    def frame(self, h, logits, g_idx):
        self.log.append(("frame", g_idx))
        audio = torch.tensor([s[min(g_idx, len(s) - 1)] for s in self.script])
        return torch.full((len(self.script),), 100 + g_idx), audio

    def advance(self, text, audio):
        self.log.append(("advance",))
        return torch.zeros(len(self.script), 1), torch.zeros(len(self.script), 1)


def test_generate_batch_bookkeeping(monkeypatch):
    dep_q, K = 4, 5
    ids = GenIds(text_pad_token=319, text_empty_token=318, semantic_pad_token=31, n_audio_codes=30, text_initial_token_id=7)
    model = types.SimpleNamespace(config=types.SimpleNamespace(dep_q=dep_q), device=torch.device("cpu"),
                                  _get_initial_token=lambda: torch.full((1, K, 1), 32))
    cfg_d = dict(n_q=K - 1)
    # (L, n_text, n_pad): prefix lengths 1, 3, 2 and maxlen = minlen = 3, 2, 5
    seqs = [R.tts_prompt(cfg_d, 6, 1, 2, 0), R.tts_prompt(cfg_d, 7, 3, 2, 1), R.tts_prompt(cfg_d, 8, 2, 1, 2)]
    ok, stop = [1, 2, 3, 4], [1, 2, 3, 30]
    # every stream ends at its own maxlen: 3, 2 and 5 frames
    script = [[ok] * 8, [ok] * 8, [ok, ok, ok, ok, ok]]
    imp = InferenceImp(None, model, "sample", 0.7, 5, 0.8, 8, "TTS", use_sampling=False, ids=ids)
    gen = _ScriptedGen(script, dep_q)
    monkeypatch.setattr(imp, "_make_gen", lambda: gen)
    outs = imp.generate_batch(seqs)
    assert [o["frames"].shape[0] for o in outs] == [3, 2, 5]
    assert all(torch.equal(o["frames"], torch.tensor([ok] * o["frames"].shape[0])) for o in outs)
    assert outs[0]["text"].tolist() == [100, 101, 102] and outs[1]["text"].tolist() == [100, 101]
    assert gen.log[0] == ("begin", 3, True) and gen.log[-1] == ("end",)
    kind, shape, lens = gen.log[1]
    assert kind == "prefill" and shape == (3, K, 4) and lens == [2, 4, 3]          # [initial frame | prefix_i]
    assert gen.tokens[0, :, 0].tolist() == [7, 32, 32, 32, 32] and gen.tokens[0, :, 2:].abs().sum() == 0
    assert torch.equal(gen.tokens[1, :, 1:4], seqs[1][:, :3])
    assert [e[1] for e in gen.log if e[0] == "frame"] == [0, 1, 2, 3, 4]
    assert sum(e[0] == "advance" for e in gen.log) == 4                            # none after the last stream's last frame
    # blanking: regime 0 for all at frame 0; at frame 1 every stream moves on (1 or 2 by pre + 1 > minlen); later writes only when a LIVE
    # stream's regime changes
    blanks = [e[1] for e in gen.log if e[0] == "blank"]
    assert blanks[0] == [[True] * dep_q] * 3
    want1 = [regime_wide(blanking_regime(p, m, 1), dep_q) for p, m in ((1, 3), (3, 2), (2, 5))]
    assert blanks[1] == want1
    pre, minlen = (1, 3, 2), (3, 2, 5)
    live_until = (3, 2, 5)
    expect, cur = [], None
    for g in range(5):
        new = [(cur[b] if cur is not None and g >= live_until[b] else blanking_regime(pre[b], minlen[b], g)) for b in range(3)]
        if new != cur:
            expect.append([regime_wide(r, dep_q) for r in new])
            cur = new
    assert blanks == expect

    # the stop rule: an id >= n_audio_codes in codebooks 3.. once g_idx > minlen ends the stream and drops that frame
    imp2 = InferenceImp(None, model, "sample", 0.7, 5, 0.8, 8, "ASR", use_sampling=False, ids=ids)
    # ASR: maxlen = n + 13, minlen = n - 13 (negative here): the rule applies from g_idx 0 on
    seq_asr = torch.full((K, 6), 3)
    seq_asr[0, :2] = 318
    gen2 = _ScriptedGen([[ok, ok, stop, ok], [ok, stop, ok, ok]], dep_q)
    monkeypatch.setattr(imp2, "_make_gen", lambda: gen2)
    outs2 = imp2.generate_batch([seq_asr, seq_asr.clone()])
    assert [o["frames"].shape[0] for o in outs2] == [2, 1]
    assert [e[1] for e in gen2.log if e[0] == "frame"] == [0, 1, 2]                 # the loop ends when every stream is done
    assert imp.generate_batch([]) == []
