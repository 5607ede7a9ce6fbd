"""Per-stream sampling, the parts that need no GPU:

1. the numpy statement of the noise (tests/helpers/stream_sampling.py): Philox4x32-10 against its known answer, the exact uniform and its
   bounds, ``-log u`` in fp64;
2. ``lm.model.check_sampling`` and the ``/api/chat`` query parser ``server.chat_sampling``: every parameter, every refusal with its reason;
3. ``SlotServerState`` over a stand-in pipeline that records calls: settings applied with the joins of a tick, grouped; a client's
   settings do not outlive it in its row; a pipeline without ``set_stream_sampling`` serves joins without ``sampling``;
4. the margins of the GPU scenarios on the CPU oracle: every sampler call of every conversation of tests/test_stream_sampling_gpu.py
   keeps MARGIN = 1e-4 -- the token equalities asserted there rest on it."""
import types

import numpy as np
import pytest
import torch

from rstnet_amd import server as S
from rstnet_amd import slots as SL
from rstnet_amd.lm.model import check_sampling
from tests.helpers import stream_sampling as H

# ------------------------------------------------------------------------------------------------------------------------ 1: the noise


def test_philox_known_answers():
    zero = H.philox4x32_10(np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32))
    assert tuple(int(v) for v in zero) == H.KAT_ZERO == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    # the two other vectors of Random123's kat_vectors: all ones, and the digits of pi
    ones = H.philox4x32_10(np.full(4, 0xFFFFFFFF, dtype=np.uint32), np.full(2, 0xFFFFFFFF, dtype=np.uint32))
    assert tuple(int(v) for v in ones) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    pi = H.philox4x32_10(np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], dtype=np.uint32), np.array([0xA4093822, 0x299F31D0], dtype=np.uint32))
    assert tuple(int(v) for v in pi) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_words_are_a_function_of_seed_frame_and_column():
    w = H.words(2 ** 63 + 5, 2 ** 32 + 7, 9)
    # column c is word c & 3 of counter (c >> 2, 0, lo32(frame), hi32(frame)) under key (lo32(seed), hi32(seed))
    for c in (0, 3, 4, 8):
        blk = H.philox4x32_10(np.array([c >> 2, 0, 7, 1], dtype=np.uint32), np.array([5, 0x80000000], dtype=np.uint32))
        assert int(w[c]) == int(blk[c & 3])
    assert np.array_equal(H.words(2 ** 63 + 5, 2 ** 32 + 7, 5), w[:5]), "a narrower row is a prefix"
    assert not np.array_equal(H.words(2 ** 63 + 5, 7, 9), w) and not np.array_equal(H.words(5, 2 ** 32 + 7, 9), w), "the high halves count"


def test_uniform_and_noise_bounds():
    u = H.uniform_of(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], dtype=np.uint32))
    assert u[0] == u[1] == 2.0 ** -24 and u[2] == 3 * 2.0 ** -24 and u[3] == 1.0 - 2.0 ** -24
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u), "the uniform is exact in fp32"
    lo, hi = -np.log(u[3]), -np.log(u[0])
    assert 0.0 < lo < 6e-8 and np.float32(lo) > 0.0 and 16.63 < hi < 16.64
    n = H.noise_f64(1, 0, 2025)
    assert n.shape == (2025,) and np.isfinite(n).all() and (n > 0).all() and n.max() <= hi
    assert 0.9 < n.mean() < 1.1, "Exp(1) has mean 1"


# ------------------------------------------------------------------------------------------------- 2: settings and the query parser

def test_check_sampling():
    assert check_sampling(dict(use_sampling=0, temp=1, temp_text="0.5", top_k=3, top_k_text=10, seed=2 ** 64 - 1), 8, 10) == \
        dict(use_sampling=False, temp=1.0, temp_text=0.5, top_k=3, top_k_text=10, seed=2 ** 64 - 1)
    assert check_sampling(dict(temp=None, top_k=8), 8, 10) == dict(top_k=8)
    for bad, why in ((dict(temp=-0.1), "temperature"), (dict(temp_text=float("inf")), "temperature"), (dict(temp=float("nan")), "temperature"),
                     (dict(top_k=0), r"1 \.\. 8"), (dict(top_k=9), r"1 \.\. 8"), (dict(top_k_text=11), r"1 \.\. 10"), (dict(top_k=2.5), "integer"),
                     (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(topk=3), "unknown sampling setting")):
        with pytest.raises(ValueError, match=why):
            check_sampling(bad, 8, 10)


@pytest.mark.parametrize("query,want", [
    ({}, None),
    ({"sr": "48000", "pcm": "s16"}, None),
    ({"temp": "0.9"}, dict(temp=0.9)),
    ({"temp_text": "0"}, dict(temp_text=0.0)),
    ({"topk": "250"}, dict(top_k=250)),
    ({"topk_text": "1"}, dict(top_k_text=1)),
    ({"seed": str(2 ** 64 - 1)}, dict(seed=2 ** 64 - 1)),
    ({"greedy": "1"}, dict(use_sampling=False)),
    ({"greedy": "0"}, dict(use_sampling=True)),
    ({"temp": "1.25", "temp_text": "0.5", "topk": "40", "topk_text": "7", "seed": "12", "greedy": "0", "pcm": "f32"},
     dict(temp=1.25, temp_text=0.5, top_k=40, top_k_text=7, seed=12, use_sampling=True)),
])
def test_chat_sampling_parses(query, want):
    assert S.chat_sampling(query, True, 250, 25) == want


@pytest.mark.parametrize("query,why", [
    ({"temp": "warm"}, "does not parse"),
    ({"temp": "-1"}, "temperature"),
    ({"temp_text": "nan"}, "temperature"),
    ({"temp": "inf"}, "temperature"),
    ({"topk": "2.5"}, "does not parse"),
    ({"topk": "0"}, r"1 \.\. 250"),
    ({"topk": "251"}, r"1 \.\. 250"),
    ({"topk_text": "26"}, r"1 \.\. 25"),
    ({"seed": "-3"}, "seed"),
    ({"seed": str(2 ** 64)}, "seed"),
    ({"seed": "0x10"}, "does not parse"),
    ({"greedy": "yes"}, "0 or 1"),
])
def test_chat_sampling_refuses(query, why):
    with pytest.raises(ValueError, match=why):
        S.chat_sampling(query, True, 250, 25)


@pytest.mark.parametrize("name", sorted(S.SAMPLING_QUERY))
def test_chat_sampling_needs_the_server_flag(name):
    with pytest.raises(ValueError, match="--per-slot-sampling"):
        S.chat_sampling({name: "1"}, False, 250, 25)
    assert S.chat_sampling({"sr": "24000"}, False, 250, 25) is None


class _Request:
    def __init__(self, query):
        self.query = query


@pytest.mark.parametrize("per_slot,query,why", [(True, {"topk": "300"}, "1 .. 250"), (True, {"temp": "hot"}, "does not parse"),
                                                (False, {"seed": "4"}, "--per-slot-sampling")])
def test_handle_chat_answers_400_before_the_upgrade(per_slot, query, why):
    import asyncio
    from aiohttp import web
    st, pipe = _slot_state(2, per_slot_sampling=per_slot)
    with pytest.raises(web.HTTPBadRequest) as e:
        asyncio.run(st.handle_chat(_Request(query)))
    assert e.value.status == 400 and why in e.value.text
    assert st.table.occupied() == [] and pipe.calls == [], "a refused client took a row or touched the pipeline"


# ------------------------------------------------------------------------------------------------------ 3: the stand-in pipeline

F_FAKE = 8
DEFAULTS = dict(use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25)


class _Mimi:
    sample_rate, frame_rate = 24000, 12.5


class _BarePipe:
    """The packed surface ``SlotServerState`` drives, recording calls; every record comes back invalid.  No ``set_stream_sampling``."""
    client_frame = F_FAKE

    def __init__(self, n):
        self.batch_size, self.record_stride = n, SL.record_stride(F_FAKE)
        self.lm_gen = types.SimpleNamespace(max_delay=1)
        self.calls = []
        self._out = torch.zeros(n, self.record_stride, dtype=torch.uint8)

    def new_staged(self):
        return torch.zeros(self.batch_size, self.record_stride, dtype=torch.uint8)

    def set_row_format(self, b, fmt):
        pass

    def reset_streams(self, rows):
        self.calls.append(("reset", list(rows)))

    def step_packed(self, staged):
        self.calls.append(("step",))
        return self._out


class _SamplingPipe(_BarePipe):
    def __init__(self, n):
        super().__init__(n)
        self.lm_gen.default_sampling = lambda: dict(DEFAULTS)

    def set_stream_sampling(self, rows, **kw):
        self.calls.append(("sampling", list(rows), kw))


def _slot_state(n=3, bare=False, **kw):
    pipe = (_BarePipe if bare else _SamplingPipe)(n)
    return S.SlotServerState(_Mimi(), None, "cpu", slots=n, pipeline=pipe, **kw), pipe


def test_two_joins_with_sampling_in_one_tick_are_grouped():
    st, pipe = _slot_state(per_slot_sampling=True)
    a = st.join("f32", sampling=dict(temp=0.5, top_k=7, seed=2 ** 63 + 1))
    b = st.join("s16", sampling=dict(use_sampling=False))
    c = st.join("f32")
    assert (a, b, c) == (0, 1, 2) and pipe.calls == [], "nothing touches the pipeline outside a tick"
    st.tick()
    # one reset for the three joins, then ONE call with every field of both clients (their own values over the defaults) and one with
    # the one seed a client named; the row that joined without settings is not mentioned; then the frame
    assert pipe.calls == [
        ("reset", [0, 1, 2]),
        ("sampling", [0, 1], dict(use_sampling=[True, False], temp=[0.5, 0.8], temp_text=[0.7, 0.7], top_k=[7, 250], top_k_text=[25, 25])),
        ("sampling", [0], dict(seed=[2 ** 63 + 1])),
        ("step",),
    ]
    st.tick()
    assert [c[0] for c in pipe.calls[4:]] == ["step"], "settings are applied once, with the join"


def test_a_clients_settings_do_not_outlive_it_in_its_row():
    st, pipe = _slot_state(2, per_slot_sampling=True)
    a = st.join("f32", sampling=dict(temp=0.0, top_k_text=1, seed=4))
    st.tick()
    st.leave(a)
    st.tick()
    del pipe.calls[:]
    assert st.join("f32") == a                    # a client without settings takes the row: the server's defaults, no seed (the reset drew one)
    st.tick()
    assert pipe.calls == [("reset", [0]), ("sampling", [0], {k: [v] for k, v in DEFAULTS.items()}), ("step",)]
    st.leave(a)
    st.tick()
    del pipe.calls[:]
    assert st.join("s16") == a                    # the row holds defaults now: nothing to undo
    st.tick()
    assert pipe.calls == [("reset", [0]), ("step",)]


def test_join_validates_before_it_takes_a_row():
    st, pipe = _slot_state(1, per_slot_sampling=True)
    with pytest.raises(ValueError, match=r"1 \.\. 250"):
        st.join("f32", sampling=dict(top_k=251))
    with pytest.raises(ValueError, match="unknown sampling setting"):
        st.join("f32", sampling=dict(topk=3))
    assert st.table.occupied() == []
    a = st.join("f32", sampling=dict(seed=1))
    st.leave(a)                                   # left before its tick: its settings go with it
    assert st.join("f32") == a
    st.tick()
    assert [c for c in pipe.calls if c[0] == "sampling"] == []


def test_joins_without_sampling_never_call_set_stream_sampling():
    st, pipe = _slot_state(2, bare=True)
    assert not hasattr(pipe, "set_stream_sampling")
    a, b = st.join("f32", sampling=None), st.join("s16")
    st.tick()
    st.leave(a)
    st.tick()
    assert st.join("f32") == a
    st.tick()
    assert [c for c in pipe.calls if c[0] == "reset"] == [("reset", [0, 1]), ("reset", [0])]


# ------------------------------------------------------------------------------------------------- 4: margins of the GPU scenarios

@pytest.mark.parametrize("limits", [False, True], ids=["plain", "limits"])
@pytest.mark.parametrize("V", H.SAMPLER_V)
def test_sampler_rows_keep_their_margins(V, limits):
    toks, worst = H.sampler_reference(V, limits)
    print(f"V = {V}, limits = {limits}: tokens {toks}, smallest margin {worst:.3e}")
    assert worst >= H.MARGIN
    lim = H.sampler_limits(V)
    assert all(0 <= t < (lim[b] if limits and b else V) for b, t in enumerate(toks))
    assert min(lim) >= H.sampler_cap(V), "a limit below the cap would make the cut row a different reference"


def test_lmgen_conversations_keep_their_margins():
    runs, worst, calls = H.lmgen_oracle_runs()
    dep_q = H.CFG["dep_q"]
    print(f"LMGen scenario: smallest margin {worst:.3e} over {calls} sampler calls")
    assert calls == 4 * H.FRAMES * (1 + dep_q), "a sampler call of a conversation was left out"
    assert worst >= H.MARGIN
    # the scenario is not vacuous: the switch changes row 2's stream (only) from its frame on, and the three rows say different things
    a, b = runs[H.SWITCH_ROW], runs["switch"]
    d = max(H.CFG["delays"])
    same = [x is None and y is None or torch.equal(x, y) for x, y in zip(a, b)]
    assert all(same[:H.SWITCH_FRAME]) and not all(same[H.SWITCH_FRAME:])
    assert all(r is None for r in runs[0][:d]) and all(r is not None for r in runs[0][d:])
    assert not all(torch.equal(x, y) for x, y in zip(runs[0][d:], runs[1][d:]))


def test_slot_server_conversations_keep_their_margins():
    worst, calls = H.slot_oracle_margin()
    print(f"slot-server scenario: smallest margin {worst:.3e} over {calls} sampler calls")
    frames = sum(t1 - t0 for _, _, t0, t1, _, _ in H.SS.CLIENTS.values())
    assert calls == frames * (1 + H.SS.cfg()["dep_q"]), "a sampler call of a conversation was left out"
    assert worst >= H.MARGIN
