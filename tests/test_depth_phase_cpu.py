"""The host logic of the depth phase of a frame, pinned on CPU tensors: ``LMGen._depth`` and ``GPTGen._depth_into`` run against
recording stand-ins of the ``ops`` entry points (tests/helpers/ops_recorder.py), and the sequence of launches they ask for -- entry
point, tensor shapes / dtypes / strides / offsets, scalars and keywords -- must equal, line by line, the sequences in
``tests/golden/depth_phase_calls.json``.

Those sequences were recorded from the tree BEFORE the two front ends shared one depth-phase executor (``RST_RECORD_DEPTH_PHASE=1``
re-records them: only ever on a tree whose depth phase is trusted), so the test states what both front ends asked of the kernels then:
``w8=`` on the stacked in-projection for LM only; head ``bias=``, ``limits=`` / ``limit_dev=`` and the ring capacity ``dep_q + 1`` for
GPT only; ``top_k`` clamped to the vocabulary for GPT only; the dense ``[B, dep_q + 1]`` copy only for a wider GPT token column.  It goes
through names that exist on both sides of that change only."""
import json
import os

import pytest
import torch

from rstnet_amd import ops, synth
from rstnet_amd.lm.generate import GPTGen
from rstnet_amd.lm.gpt import GPT, Config
from rstnet_amd.lm.model import LMGen, LMModel
from tests.helpers.ops_recorder import OpsRecorder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_phase_calls.json")
TOP_K = 5


def _expected(case: str, log):
    if os.environ.get("RST_RECORD_DEPTH_PHASE", "") not in ("", "0"):
        data = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        data[case] = log
        with open(GOLDEN, "w") as f:
            json.dump(dict(sorted(data.items())), f, indent=0)
    return json.load(open(GOLDEN))[case]


def _pretend_device_tensors(monkeypatch):
    """The persistent route is only taken for device tensors (``LMGen._depth`` asks ``h_t.is_cuda``, the pointer tables assert it of
    every weight): the stand-ins launch nothing, so the CPU tensors of this test may answer yes."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))


def _launches(log):
    """The lines that stand for launches (the rest are the route's questions to the library)."""
    return [l for l in log if l.split("(")[0] not in ("depth_frame_enabled", "depth_frame_supported", "gemv_attn_supported")]


def _noise(B: int, n: int, sampling: bool):
    # as in a frame: the depth samplers' columns of a wider per-frame draw (so the row stride is not the width)
    return torch.ones(B, 3 + n)[:, 3:] if sampling else None


@pytest.fixture(scope="module")
def lm():
    cfg = dict(synth.LM_TINY)
    return LMModel.from_state_dict(synth.lm_state_dict(cfg, 3), cfg), cfg


@pytest.fixture(scope="module")
def gpt():
    cfg = Config.from_dict(synth.GPT_TINY_GQA)
    return GPT.from_state_dict(synth.gpt_state_dict(synth.GPT_TINY_GQA, 5), cfg), cfg


@pytest.mark.parametrize("sampling", [True, False], ids=["sampled", "greedy"])
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "chain"])
def test_lmgen_depth_asks_for_the_same_launches(lm, monkeypatch, persistent, B, sampling):
    model, cfg = lm
    rec = OpsRecorder(depth_frame=persistent).install(monkeypatch, ops)
    if persistent:
        _pretend_device_tensors(monkeypatch)
    gen = LMGen(model, use_sampling=sampling, top_k=TOP_K)
    with gen.streaming(B):
        tokens = torch.zeros(B, cfg["dep_q"] + 1, dtype=torch.long)
        if persistent:
            model.depth_frame_tables()      # cached on the (shared) model: built here so that no case's log depends on which ran first
        rec.log.clear()
        gen._depth(tokens, torch.zeros(B, cfg["dim"]), _noise(B, cfg["dep_q"] * TOP_K, sampling))
        log = list(rec.log)
        if persistent and B <= 2:
            assert gen._streaming_state.tables is model.depth_frame_tables()      # kept alive with the session's frame graph
    for line in log:
        print(line)
    one_launch = persistent and B <= 2
    assert [l.split("(")[0] for l in log].count("depth_decode_frame") == int(one_launch)
    if not one_launch and B <= 2:
        assert len(_launches(log)) == 17      # stacked in-projection + 2 steps x (2 layers x 3 launches + head + sampler)
    assert log == _expected(f"lm-{'persistent' if persistent else 'chain'}-B{B}-{'sampled' if sampling else 'greedy'}", log)


@pytest.mark.parametrize("wide", [False, True], ids=["dep_q+1", "n_q+1"])
@pytest.mark.parametrize("sampling", [True, False], ids=["sampled", "greedy"])
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "chain"])
def test_gptgen_depth_asks_for_the_same_launches(gpt, monkeypatch, persistent, B, sampling, wide):
    model, cfg = gpt
    rec = OpsRecorder(depth_frame=persistent).install(monkeypatch, ops)
    if persistent:
        _pretend_device_tensors(monkeypatch)
    gen = GPTGen(model, use_sampling=sampling, top_k=TOP_K, n_audio_codes=30)
    gen.begin(B)
    try:
        tokens = torch.zeros(B, (cfg.n_q if wide else cfg.dep_q) + 1, dtype=torch.long)      # `step`'s session column | `frame`'s buffer
        if persistent:
            model.depth_frame_tables()      # (as above)
        rec.log.clear()
        gen._depth_into(tokens, torch.zeros(B, cfg.n_embd), _noise(B, cfg.dep_q * TOP_K, sampling))
        log = list(rec.log)
    finally:
        gen.end()
    for line in log:
        print(line)
    one_launch = persistent and B <= 2
    assert [l.split("(")[0] for l in log].count("depth_decode_frame") == int(one_launch)
    if not one_launch and B <= 2:
        assert len(_launches(log)) == 25      # as above with 3 steps
    name = f"gpt-{'persistent' if persistent else 'chain'}-B{B}-{'sampled' if sampling else 'greedy'}-{'wide' if wide else 'dense'}"
    assert log == _expected(name, log)
