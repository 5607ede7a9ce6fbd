"""The host side of the slot server (rstnet_amd/slots.py, SlotServerState of rstnet_amd/server.py) without a GPU: the slot table, the
tick rule, the inbox, the two record layouts, the numpy statement of the egress, the driver API over a stand-in pipeline that echoes its
input, the websocket layer on localhost, and the margins of the oracles' greedy decisions on the inputs of tests/test_slot_server_gpu.py."""
import argparse
import asyncio
import types

import numpy as np
import pytest
import torch

from rstnet_amd import server as S
from rstnet_amd import slots as SL
from tests.helpers import slot_server as H


# ------------------------------------------------------------------------------------------------------------------ table, clock, inbox

def test_slot_table_lowest_free_row_exhaustion_and_reuse():
    t = SL.SlotTable(3)
    assert [t.acquire(), t.acquire(), t.acquire()] == [0, 1, 2] and t.acquire() is None
    assert t.rows(SL.JOINING) == [0, 1, 2] and t.occupied() == [0, 1, 2]
    t.mark_live(1)
    assert t.state(1) == SL.LIVE and t.rows(SL.LIVE) == [1]
    with pytest.raises(ValueError):
        t.mark_live(1)                                  # only a joining row becomes live
    t.release(1)
    t.release(0)
    assert t.state(1) == SL.FREE and t.occupied() == [2]
    assert t.acquire() == 0 and t.state(0) == SL.JOINING and t.acquire() == 1 and t.acquire() is None
    with pytest.raises(ValueError):
        SL.SlotTable(1).release(0)
    with pytest.raises(ValueError):
        SL.SlotTable(0)


@pytest.mark.parametrize("ready, occupied, elapsed, want", [
    ([], [], 0.0, False), ([], [], 1.0, False),                         # no occupied row: never due
    ([0], [0], 0.0, True),                                              # everyone has a frame: at once
    ([0, 2], [0, 2], 0.0, True),
    ([0], [0, 2], 0.0, False), ([0], [0, 2], 0.0799, False),            # one late row: only when the period has passed
    ([0], [0, 2], 0.08, True), ([0], [0, 2], 0.5, True),
    ([], [1], 0.01, False), ([], [1], 0.08, True),
    ([0, 1, 2], [1], 0.0, True),                                        # frames of rows that are not occupied do not matter
])
def test_tick_due_truth_table(ready, occupied, elapsed, want):
    assert SL.tick_due(ready, occupied, elapsed, 0.08) is want


def test_inbox_drops_the_oldest_and_counts():
    box = SL.Inbox(frame_bytes=4, max_backlog=2)
    box.push(b"\x01\x01\x01")
    assert len(box) == 0 and box.pop() is None          # a partial frame waits
    box.push(b"\x01" + b"\x02" * 4 + b"\x03" * 4 + b"\x04\x04")
    assert len(box) == 2 and box.dropped == 1           # three whole frames arrived: the oldest went
    assert box.pop() == b"\x02" * 4 and box.pop() == b"\x03" * 4 and box.pop() is None
    box.push(b"\x04\x04")
    assert box.pop() == b"\x04" * 4 and box.dropped == 1 and box.underruns == 0
    assert SL.Inbox(4).max_backlog == 4
    with pytest.raises(ValueError):
        SL.Inbox(4, 0)


# ------------------------------------------------------------------------------------------------------------------ the record layouts

def test_record_stride():
    assert SL.record_stride(5) == 48 and SL.record_stride(1920) == 7696
    assert SL.record_stride(882) == 3552 and (16 + 4 * 882) % 16 == 8      # the rounding is what keeps row 1 on a 16-byte boundary


def test_pack_staged_and_parse_records_round_trip():
    F, B = 5, 4
    rng = np.random.default_rng(0)
    f32 = rng.standard_normal(F).astype("<f4").tobytes()
    s16 = rng.integers(-32768, 32768, F).astype("<i2").tobytes()
    fmt = [SL.FMT_F32, SL.FMT_S16, SL.FMT_FREE, SL.FMT_F32]
    buf = np.full((B, SL.record_stride(F)), 0xEE, dtype=np.uint8)
    SL.pack_staged(buf, [f32, s16, None, None], fmt, F)
    head = buf[:, :4].view("<i4")[:, 0]
    assert head.tolist() == [1, 1, 0, 0]
    assert buf[0, 16:16 + 4 * F].tobytes() == f32 and buf[1, 16:16 + 2 * F].tobytes() == s16
    got = SL.ingress_reference(buf, fmt, F)
    assert np.array_equal(got[0, 0], np.frombuffer(f32, "<f4"))
    assert np.array_equal(got[1, 0], np.frombuffer(s16, "<i2").astype(np.float32) / 32768.0)
    assert not got[2:].any()
    with pytest.raises(ValueError, match="bytes"):
        SL.pack_staged(buf, [s16, None, None, None], fmt, F)               # an s16 frame in an f32 row
    # the egress side: records written by the reference, read back by the parser
    wav = rng.standard_normal((B, 1, F)).astype(np.float32)
    tokens = np.arange(B * 3, dtype=np.int64).reshape(B, 3) + 40
    rec = SL.egress_reference(wav, tokens, [5, 5, 5, 1], 1, fmt, F)
    parsed = SL.parse_records(rec, F)
    assert parsed[2] is None and parsed[3] is None
    assert parsed[0] == (40, S.PcmFramer(F, "f32").encode(wav[0, 0])) and parsed[1] == (43, S.PcmFramer(F, "s16").encode(wav[1, 0]))


@pytest.mark.parametrize("F", [5, 882])
def test_egress_reference_is_pcmframer_encode_per_row(F):
    rng = np.random.default_rng(F)
    B, max_delay = 4, 1
    wav = (0.7 * rng.standard_normal((B, 1, F))).astype(np.float32)
    wav[0, 0, :2] = [2.0, -3.0]
    wav[1, 0, :3] = [2.0, -3.0, np.nan]
    tokens = rng.integers(0, 2048, (B, 9)).astype(np.int64)
    fmt = [SL.FMT_F32, SL.FMT_S16, SL.FMT_FREE, SL.FMT_S16]
    offsets = [2, 2, 9, 1]                                                  # row 3 is still inside its delay
    rec = SL.egress_reference(wav, tokens, offsets, max_delay, fmt, F)
    REC = SL.record_stride(F)
    assert rec.shape == (B, REC) and rec.dtype == np.uint8
    head = rec[:, :16].view("<i4")
    assert head.tolist() == [[1, int(tokens[0, 0]), 4 * F, 0], [1, int(tokens[1, 0]), 2 * F, 0], [0, -1, 0, 0], [0, -1, 0, 0]]
    assert rec[0, 16:16 + 4 * F].tobytes() == S.PcmFramer(F, "f32").encode(wav[0, 0]) and not rec[0, 16 + 4 * F:].any()
    clean = wav[1, 0].copy()
    clean[2] = 0.0                                                          # NaN is defined as 0
    assert rec[1, 16:16 + 2 * F].tobytes() == S.PcmFramer(F, "s16").encode(clean) and not rec[1, 16 + 2 * F:].any()
    assert np.frombuffer(rec[1, 16:22].tobytes(), "<i2").tolist() == [32767, -32767, 0]
    assert not rec[2, 16:].any() and not rec[3, 16:].any()


# ------------------------------------------------------------------------------------------------------------------ the driver API

F_FAKE = 8


class _Mimi:
    sample_rate, frame_rate = 24000, 12.5


class _EchoPipe:
    """The pipeline's packed surface.  A row echoes the frame it was fed, in its own transport (silence for ``present = 0``), with a text
    token 100 * row + frames since its reset; its records are valid once it is past ``max_delay`` frames since its reset, as the device
    counters would say.  Rows start far past the delay (a server that has warmed up) until they are reset."""
    client_frame, max_delay = F_FAKE, 1

    def __init__(self, n):
        self.batch_size, self.record_stride = n, SL.record_stride(F_FAKE)
        self.lm_gen = types.SimpleNamespace(max_delay=self.max_delay)
        self.fmt, self.frames = [SL.FMT_FREE] * n, [100] * n
        self.calls, self.seen = [], []
        self._out = torch.zeros(n, self.record_stride, dtype=torch.uint8)

    def new_staged(self):
        return torch.zeros(self.batch_size, self.record_stride, dtype=torch.uint8)

    def set_row_format(self, b, fmt):
        self.calls.append(("fmt", b, fmt))
        self.fmt[b] = fmt

    def reset_streams(self, rows):
        self.calls.append(("reset", list(rows)))
        for b in rows:
            self.frames[b] = 0

    def step_packed(self, staged):
        buf = staged.numpy()
        self.seen.append(buf[:, :4].view("<i4")[:, 0].tolist())
        pcm = SL.ingress_reference(buf, self.fmt, F_FAKE)
        self.frames = [n + 1 for n in self.frames]
        tokens = np.array([[100 * b + self.frames[b]] for b in range(self.batch_size)], dtype=np.int64)
        self._out.numpy()[:] = SL.egress_reference(pcm, tokens, self.frames, self.max_delay, self.fmt, F_FAKE)
        return self._out


def _slot_state(n=3, **kw):
    pipe = _EchoPipe(n)
    return S.SlotServerState(_Mimi(), None, "cpu", slots=n, pipeline=pipe, **kw), pipe


def _f32(value):
    return np.full(F_FAKE, value, dtype="<f4").tobytes()


def _s16(value):
    return np.full(F_FAKE, value, dtype="<i2").tobytes()


def _s16_echo(value):
    """What an s16 sample comes back as: in through x / 32768, out through trunc(x * 32767)."""
    return S.PcmFramer(F_FAKE, "s16").encode(np.full(F_FAKE, value, dtype=np.float32) / 32768.0)


def test_period_comes_from_the_codec():
    st, _ = _slot_state()
    assert st.period == pytest.approx(0.08) and st.F == F_FAKE and st.max_delay == 1


def test_two_joins_inside_one_tick_are_one_reset():
    st, pipe = _slot_state()
    a, b = st.join("f32"), st.join("s16")
    assert (a, b) == (0, 1) and st.table.rows(SL.JOINING) == [0, 1]
    assert pipe.calls == []                                          # nothing touches the pipeline outside a tick
    st.push(a, _f32(0.25))
    st.push(b, _s16(1000))
    out = st.tick()
    assert [c for c in pipe.calls if c[0] == "reset"] == [("reset", [0, 1])]
    assert ("fmt", 0, SL.FMT_F32) in pipe.calls and ("fmt", 1, SL.FMT_S16) in pipe.calls
    assert st.table.rows(SL.LIVE) == [0, 1] and out == {}            # frame 1 of both rows: inside the delay
    st.push(a, _f32(0.5))
    st.push(b, _s16(-2000))
    out = st.tick()
    assert out == {0: [(S.KIND_AUDIO, _f32(0.5)), (S.KIND_TEXT, b"<2>")], 1: [(S.KIND_AUDIO, _s16_echo(-2000)), (S.KIND_TEXT, b"<102>")]}
    assert len([c for c in pipe.calls if c[0] == "reset"]) == 1
    with pytest.raises(ValueError):
        st.join("opus")


def test_a_left_row_is_reset_when_it_is_acquired_again_not_before():
    st, pipe = _slot_state(2)
    a = st.join("f32")
    st.tick()
    st.leave(a)
    assert pipe.calls == [("reset", [0]), ("fmt", 0, SL.FMT_F32)]    # leaving issues no pipeline call by itself
    assert st.tick() == {}
    assert pipe.calls[2:] == [("fmt", 0, SL.FMT_FREE)]               # the next tick frees the row's format word; no reset
    st.tick()
    assert len(pipe.calls) == 3
    c = st.join("s16")
    assert c == 0
    st.tick()
    assert pipe.calls[3:] == [("reset", [0]), ("fmt", 0, SL.FMT_S16)]
    # left and taken again between two ticks: one reset, the new format, never the free word
    st.leave(c)
    d = st.join("f32")
    assert d == 0
    st.tick()
    assert pipe.calls[5:] == [("reset", [0]), ("fmt", 0, SL.FMT_F32)]


def test_underrun_feeds_silence_and_is_counted():
    st, pipe = _slot_state(2)
    a = st.join("f32")
    st.push(a, _f32(0.5))
    st.tick()
    assert pipe.seen[-1] == [1, 0] and st.underruns(a) == 0
    out = st.tick()                                                  # nothing queued: present = 0, silence, counted
    assert pipe.seen[-1] == [0, 0] and st.underruns(a) == 1
    assert out == {0: [(S.KIND_AUDIO, _f32(0.0)), (S.KIND_TEXT, b"<2>")]}
    st.push(a, _f32(0.5) * 6)                                        # six frames at once: the two oldest are dropped (max_backlog 4)
    assert st.dropped(a) == 2
    st.tick()
    assert pipe.seen[-1] == [1, 0] and st.underruns(a) == 1
    # a row whose join is applied by this tick owes no frame yet
    b = st.join("s16")
    st.tick()
    assert st.underruns(b) == 0
    st.tick()
    assert st.underruns(b) == 1


def test_free_rows_never_return_anything():
    st, pipe = _slot_state(2)
    st.warmup()
    assert st.ticks == pipe.max_delay + 3 and pipe.calls == []
    a = st.join("f32")
    st.tick()
    st.push(a, _f32(0.1))
    assert sorted(st.tick()) == [0]


# ------------------------------------------------------------------------------------------------------------------ sockets

def _run(coro):
    loop = asyncio.new_event_loop()
    try:
        return loop.run_until_complete(coro)
    finally:
        loop.close()


async def _audio(ws, n, timeout=5.0):
    got = []
    while len(got) < n:
        msg = await asyncio.wait_for(ws.receive_bytes(), timeout=timeout)
        if msg[0] == S.KIND_AUDIO:
            got.append(msg[1:])
    return got


def test_websocket_two_clients_at_once_third_refused_then_served():
    from aiohttp import WSServerHandshakeError
    from aiohttp.test_utils import TestClient, TestServer

    async def scenario():
        st, pipe = _slot_state(2)
        st.warmup()
        client = TestClient(TestServer(S.make_app(st)))
        await client.start_server()
        try:
            ws1 = await client.ws_connect("/api/chat")
            ws2 = await client.ws_connect("/api/chat?pcm=s16")
            assert (await asyncio.wait_for(ws1.receive_bytes(), 5.0)) == b"\x00"
            assert (await asyncio.wait_for(ws2.receive_bytes(), 5.0)) == b"\x00"          # both talk at the same time: no lock
            # a third client: refused before the upgrade, with the reason
            with pytest.raises(WSServerHandshakeError) as e:
                await client.ws_connect("/api/chat")
            assert e.value.status == 503
            resp = await client.get("/api/chat")
            assert resp.status == 503 and "slots" in await resp.text()
            # four frames each, in pieces that do not line up with frames; each gets only its own audio back
            raw1 = b"".join(_f32(0.125 * (i + 1)) for i in range(4))
            raw2 = b"".join(_s16(-100 * (i + 1)) for i in range(4))
            for a in range(0, len(raw1), 24):
                await ws1.send_bytes(b"\x01" + raw1[a:a + 24])
            for a in range(0, len(raw2), 10):
                await ws2.send_bytes(b"\x01" + raw2[a:a + 10])
            got1, got2 = await _audio(ws1, 2), await _audio(ws2, 2)
            assert all(len(p) == 4 * F_FAKE for p in got1) and all(len(p) == 2 * F_FAKE for p in got2)
            mine1 = {_f32(0.125 * (i + 1)) for i in range(4)} | {_f32(0.0)}
            mine2 = {_s16_echo(-100 * (i + 1)) for i in range(4)} | {_s16(0)}
            assert set(got1) <= mine1 and set(got2) <= mine2
            assert any(p != _f32(0.0) for p in got1) and any(p != _s16(0) for p in got2)
            # one leaves: its row serves the next client, after a reset
            await ws1.close()
            for _ in range(200):
                if st.table.state(0) == SL.FREE:
                    break
                await asyncio.sleep(0.005)
            assert st.table.state(0) == SL.FREE
            resets = len([c for c in pipe.calls if c[0] == "reset"])
            ws3 = await client.ws_connect("/api/chat")
            assert (await asyncio.wait_for(ws3.receive_bytes(), 5.0)) == b"\x00"
            assert [c for c in pipe.calls if c[0] == "reset"][resets:] == [("reset", [0])]
            await ws3.send_bytes(b"\x01" + _f32(0.75) * 3)
            assert set(await _audio(ws3, 1)) <= {_f32(0.75), _f32(0.0)}
            await ws3.close()
            await ws2.close()
        finally:
            await client.close()

    _run(scenario())


def test_websocket_refusals_before_the_upgrade():
    from aiohttp.test_utils import TestClient, TestServer

    async def scenario():
        st, pipe = _slot_state(2)
        client = TestClient(TestServer(S.make_app(st)))
        await client.start_server()
        try:
            for q, why in (("sr=48000", "24000 Hz"), ("sr=abc", "positive integer"), ("pcm=mp3", "unknown pcm format")):
                resp = await client.get("/api/chat?" + q)
                assert resp.status == 400 and why in await resp.text(), q
            assert st.table.occupied() == [] and pipe.calls == []          # no row was claimed for them
            ws = await client.ws_connect("/api/chat?sr=24000&pcm=f32")     # the server's own rate, named
            assert (await asyncio.wait_for(ws.receive_bytes(), 5.0)) == b"\x00"
            await ws.close()
        finally:
            await client.close()

    _run(scenario())


def test_slots_absent_builds_a_plain_server_state(monkeypatch):
    made = []
    monkeypatch.setattr(S, "ServerState", lambda *a, **k: made.append(("plain", k)) or "plain")
    monkeypatch.setattr(S, "SlotServerState", lambda *a, **k: made.append(("slots", k)) or "slots")
    assert S.make_state(None, None, "cpu", argparse.Namespace()) == "plain"                  # (a caller's namespace from before --slots)
    assert S.make_state(None, None, "cpu", argparse.Namespace(slots=None, client_rate=None)) == "plain"
    assert S.make_state(None, None, "cpu", argparse.Namespace(slots=4, client_rate=48000)) == "slots"
    assert [m[0] for m in made] == ["plain", "plain", "slots"] and made[-1][1]["slots"] == 4 and made[-1][1]["client_rate"] == 48000
    monkeypatch.undo()
    with pytest.raises(ValueError, match="1 .. 64"):
        S.SlotServerState(_Mimi(), None, "cpu", slots=65, pipeline=_EchoPipe(65))
    with pytest.raises(SystemExit):
        S.main(["--synthetic", "--client-rate", "48000"])                                    # --client-rate belongs to --slots
    with pytest.raises(SystemExit):
        S.main(["--synthetic", "--slots", "65"])


# ------------------------------------------------------------------------------------------------------------------ the GPU scenario's inputs

def test_oracle_margins_of_the_gpu_scenario():
    """tests/test_slot_server_gpu.py compares token streams of two GPU runs with different neighbours: no greedy decision on these inputs
    may be near a tie."""
    margin = H.oracle_margin()
    print(f"smallest greedy margin of the slot-server scenario: {margin:.3e}")
    assert margin >= H.MARGIN, margin
