"""The host logic of the temporal pass of both LM families, pinned on CPU tensors: ``LMModel.forward_text`` / ``forward`` and
``LLAMAStreamingTransformer.run`` / ``GPT.forward`` run against recording stand-ins of the ``ops`` entry points
(tests/helpers/ops_recorder.py), and the launches they ask for -- entry point, tensor shapes / dtypes / strides / offsets, scalars and
keywords -- must equal, line by line, the sequences in ``tests/golden/temporal_pass_calls.json``; after every call the host counter
``offset_cpu`` must stand where the positions fed so far put it.

Those sequences were recorded from the tree BEFORE the two families shared one ring state and one layer walker
(``RST_RECORD_TEMPORAL_PASS=1`` re-records them: only ever on a tree whose temporal pass is trusted), so the test states what each
front end asked of the kernels then: ``heads=None`` / ``freqs=None`` / ``rope_dims=0`` for the LM, ``heads=H`` / the litgpt frequency
table / ``rope_dims=rope_n_elem`` for GPT; the step rotation table on long rings only; ``packed`` by batch (and not under fp8 for GPT);
stored weight copies on the LM's temporal layers only; the append-first route for GPT only; one persistent launch instead of the chain
when the library wants it.  The fixture stores every distinct line once and a call as a list of indices into them."""
import json
import os

import pytest
import torch

from rstnet_amd import ops, synth
from rstnet_amd.lm import gpt as G
from rstnet_amd.lm import model as M
from tests.helpers.ops_recorder import OpsRecorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_pass_calls.json")
QUESTIONS = ("gemv_attn_supported", "temporal_frame_wanted", "temporal_frame_supported", "persistent_epoch")
BF16 = torch.bfloat16


def _launches(log):
    """The lines that stand for launches (the rest are the route's questions to the library)."""
    return [l for l in log if l.split("(")[0] not in QUESTIONS]


def _expected(case: str, calls):
    """``calls``: one list of lines per call of the case -> what the fixture holds for it, in the same form."""
    if os.environ.get("RST_RECORD_TEMPORAL_PASS", "") not in ("", "0"):
        data = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {"lines": [], "cases": {}}
        index = {line: i for i, line in enumerate(data["lines"])}
        for line in (l for call in calls for l in call):
            if line not in index:
                index[line] = len(data["lines"])
                data["lines"].append(line)
        data["cases"][case] = [[index[l] for l in call] for call in calls]
        data["cases"] = dict(sorted(data["cases"].items()))
        with open(GOLDEN, "w") as f:
            json.dump(data, f, indent=0)
    data = json.load(open(GOLDEN))
    return [[data["lines"][i] for i in call] for call in data["cases"][case]]


class _Calls:
    """Collects, per call, the launches the recorder saw since the last one."""

    def __init__(self, rec):
        self.rec, self.calls = rec, []
        rec.log.clear()

    def take(self):
        self.calls.append(_launches(self.rec.log))
        for line in self.calls[-1]:
            print(line)
        print("--")
        self.rec.log.clear()
        return self.calls[-1]


def _names(call):
    return [l.split("(")[0] for l in call]


# ------------------------------------------------------------------------------------------------------------------------------- LM
def _lm(context: int, weights: str = "bf16"):
    cfg = dict(synth.LM_TINY, context=context)
    model = M.LMModel.from_state_dict(synth.lm_state_dict(cfg, 3), cfg, kv_dtype=BF16)
    if weights != "bf16":
        # stand-in copies of the shapes the device quantisers return (they do not run here): fp8 = bytes [N, K] + one fp32 scale per row,
        # MXFP4 = two codes per byte [N, K / 2] + one scale byte per block of 32
        as4 = {(id(m), n) for m, n in model._layer_weights()} if weights == "mxfp4" else set()
        for mod, name in model._covered_weights():
            N, K = getattr(mod, name).shape
            if (id(mod), name) in as4:
                M._attach_copy(mod, name, "4", torch.zeros(N, K // 2, dtype=torch.uint8), torch.zeros(N, K // 32, dtype=torch.uint8))
            else:
                M._attach_copy(mod, name, "8", torch.zeros(N, K, dtype=torch.uint8), torch.zeros(N, dtype=torch.float32))
        model.weight_dtype = model.transformer.weight_dtype = weights
    return model, cfg


def _lm_tokens(cfg, B, S):
    return torch.zeros(B, cfg["n_q"] + 1, S, dtype=torch.long)


@pytest.mark.parametrize("weights,B", [("bf16", 1), ("bf16", 2), ("bf16", 4), ("fp8", 1), ("fp8", 4), ("mxfp4", 1), ("mxfp4", 4)])
@pytest.mark.parametrize("context", [10, 96])
def test_lm_streaming_asks_for_the_same_launches(monkeypatch, context, weights, B):
    rec = OpsRecorder().install(monkeypatch, ops, temporal=True)
    model, cfg = _lm(context, weights)
    L = cfg["num_layers"]
    calls, at = _Calls(rec), 0
    with model.streaming(B):
        st = model.transformer._streaming_state
        assert st.k[0].dtype == (BF16 if context > 64 else torch.float32)      # rings of <= 64 slots silently stay fp32
        for S in (1, 7, 7, 1):      # at context 10 the second 7 crosses the ring wrap
            out, logits = model.forward_text(_lm_tokens(cfg, B, S))
            assert out.shape == (B, S, cfg["dim"]) and logits.shape[:3] == (B, 1, S)
            at += S
            assert st.offset_cpu == at
            names = _names(calls.take())
            assert names.count("lm_attn_decode") == (L if S == 1 else 0)
            assert names.count("lm_attn_prefill") == names.count("lm_ring_append") == (0 if S == 1 else L)
            assert "lm_rope_append" not in names and "attention" not in names      # the LM never appends first
            assert names.count("lm_rope_table") == int(S == 1 and context > 64)
    assert calls.calls == _expected(f"lm-ctx{context}-{weights}-B{B}", calls.calls)


@pytest.mark.parametrize("B", [1, 4])
def test_lm_forward_asks_for_the_same_launches(monkeypatch, B):
    """Outside ``streaming()``: the multi-position pass on throw-away rings, then the teacher-forced depth pass (``forward_local``)."""
    rec = OpsRecorder().install(monkeypatch, ops, temporal=True)
    model, cfg = _lm(10)
    calls = _Calls(rec)
    audio, text = model.forward(_lm_tokens(cfg, B, 3))
    assert audio.shape == (B, 3, cfg["dep_q"], cfg["card"]) and text.shape[:2] == (B, 3)
    assert model.transformer._streaming_state is None and model.depformer._streaming_state is None
    names = _names(calls.take())
    assert "gemv_embed" not in names      # forward_local feeds the depth transformer a plain x
    assert calls.calls == _expected(f"lm-forward-B{B}", calls.calls)


def test_lm_persistent_step_is_one_launch(monkeypatch):
    rec = OpsRecorder(temporal_frame=True).install(monkeypatch, ops, temporal=True)
    model, cfg = _lm(96)
    calls = _Calls(rec)
    with model.streaming(1):
        st = model.transformer._streaming_state
        for n in (1, 2):
            model.forward_text(_lm_tokens(cfg, 1, 1))
            assert st.offset_cpu == n
            names = _names(calls.take())
            assert names.count("temporal_decode_frame") == 1 and names.count("TemporalFrameTables") == int(n == 1)
            assert not {"lm_attn_decode", "gemv_attn", "lm_gated_pair"} & set(names)      # no chain launches
    assert calls.calls == _expected("lm-persistent-B1", calls.calls)


# ------------------------------------------------------------------------------------------------------------------------------ GPT
GPT_CFGS = {"gqa": synth.GPT_TINY_GQA, "mha": synth.GPT_TINY_MHA}


def _gpt(name: str, merge: bool):
    cfg_d = dict(GPT_CFGS[name])
    return G.GPT.from_state_dict(synth.gpt_state_dict(cfg_d, 5), G.Config.from_dict(cfg_d), merge_lora=merge), cfg_d


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("ring", ["f32x10", "f32x10-fp8", "bf16x96"])
@pytest.mark.parametrize("merge", [True, False], ids=["merged", "unmerged"])
@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_gpt_run_asks_for_the_same_launches(monkeypatch, name, merge, ring, B):
    rec = OpsRecorder().install(monkeypatch, ops, temporal=True)
    monkeypatch.setattr(M, "PREFILL_CHUNK", 4)
    model, cfg_d = _gpt(name, merge)
    model.use_fp8(ring.endswith("fp8"))
    tr, L, E = model.transformer, cfg_d["n_layer"], cfg_d["n_embd"]
    st = tr._make_state(B, 96, kv_dtype=BF16) if ring == "bf16x96" else tr._make_state(B, 10)
    calls, at = _Calls(rec), 0
    # fp32 ring of 10: a step | positions 1 .. 6 append first | 7 .. 13 in chunks of 4 and 3 across the wrap | a step
    # bf16 ring of 96: never appends first, so the 6 positions are chunks of 4 and 2 as well
    append_first = {6} if ring != "bf16x96" else set()
    for T in (1, 6, 7, 1):
        y = tr.run(torch.zeros(B * T, E), B, T, st)
        assert y.shape == (B * T, E)
        at += T
        assert st.offset_cpu == at
        names = _names(calls.take())
        chunks = 0 if T == 1 or T in append_first else -(-T // 4)
        assert names.count("lm_attn_decode") == (L if T == 1 else 0)
        assert names.count("lm_rope_append") == names.count("attention") == (L if T in append_first else 0)
        assert names.count("lm_attn_prefill") == names.count("lm_ring_append") == chunks * L
        assert names.count("lm_rope_table") == int(T == 1 and ring == "bf16x96")
        assert names.count("lm_gated_pair") == (max(chunks, 1) * L if merge or not cfg_d["lora_mlp"] else 0)
        assert names[-1] == "rmsnorm"
    assert calls.calls == _expected(f"gpt-{name}-{'merged' if merge else 'unmerged'}-{ring}-B{B}", calls.calls)


@pytest.mark.parametrize("ring", ["f32x10", "bf16x96"])
def test_gpt_one_position_tail_is_a_decode_step(monkeypatch, ring):
    """A chunked call whose last chunk holds ONE position (T = 5 at chunk 4, behind 8 positions): the tail takes the launches of a lone
    step -- the rotation table on the long ring, then ``lm_attn_decode`` per layer -- not the prefill kernels at Tc = 1."""
    rec = OpsRecorder().install(monkeypatch, ops, temporal=True)
    monkeypatch.setattr(M, "PREFILL_CHUNK", 4)
    model, cfg_d = _gpt("gqa", True)
    tr, L, E = model.transformer, cfg_d["n_layer"], cfg_d["n_embd"]
    st = tr._make_state(2, 96, kv_dtype=BF16) if ring == "bf16x96" else tr._make_state(2, 10)
    st.pos.fill_(8)
    st.offset_cpu = 8
    calls = _Calls(rec)
    assert tr.run(torch.zeros(2 * 5, E), 2, 5, st).shape == (2 * 5, E) and st.offset_cpu == 13
    names = _names(calls.take())
    assert names.count("lm_attn_prefill") == names.count("lm_ring_append") == L and names.count("lm_attn_decode") == L
    assert names.count("lm_rope_table") == int(ring == "bf16x96")
    assert names.index("lm_attn_decode") > max(i for i, n in enumerate(names) if n == "lm_ring_append")
    assert calls.calls == _expected(f"gpt-gqa-merged-{ring}-tail1", calls.calls)


@pytest.mark.parametrize("merge", [True, False], ids=["merged", "unmerged"])
@pytest.mark.parametrize("name", ["gqa", "mha"])
def test_gpt_forward_asks_for_the_same_launches(monkeypatch, name, merge):
    """Outside ``streaming()``: the T positions on a ring that never fills, then the teacher-forced depth pass (``forward_local``)."""
    rec = OpsRecorder().install(monkeypatch, ops, temporal=True)
    model, cfg_d = _gpt(name, merge)
    calls = _Calls(rec)
    audio, text = model.forward(torch.zeros(2, cfg_d["n_q"] + 1, 5, dtype=torch.long))
    assert audio.shape == (2, 5, cfg_d["dep_q"], cfg_d["audio_card"]) and text.shape[:2] == (2, 5)
    assert model.transformer._streaming_state is None and model.codecformer._streaming_state is None
    names = _names(calls.take())
    assert "gemv_embed" not in names and names.count("lm_rope_append") == cfg_d["n_layer"]
    assert calls.calls == _expected(f"gpt-forward-{name}-{'merged' if merge else 'unmerged'}", calls.calls)
