"""The slot server on the GPU: the scenario of tests/helpers/slot_server.py (three rows, 14 ticks: A joins, B joins later in s16 and
misses a frame, A leaves, C takes A's row) through ``SlotServerState``'s driver API over the real Mimi codec and the tiny 16-stream LM.
Every conversation's messages -- audio payload bytes and text pieces, in order -- must equal, byte for byte, those of a NEW
``StreamingPipeline(per_stream=True)`` of the same batch size in which that row is fed the same frames from its own frame 0 (silence
where it under-ran), taken from ``step`` and encoded by ``PcmFramer.encode``.  The other rows of such a reference run carry other audio
than they did in the server run, so the equality also shows that a row's neighbours do not matter.

Greedy (``use_sampling=False``): the noise of a sampled frame is drawn for the whole batch from one generator, so a sampled row cannot
be reproduced on its own.  Token equality between the runs rests on the margins tests/test_slot_server_cpu.py holds for these inputs.

Then one end-to-end case over websockets: two clients at once on a server of two rows, a third refused with 503."""
import asyncio
import functools

import numpy as np
import pytest
import torch

from rstnet_amd import server as S
from rstnet_amd import slots as SL
from rstnet_amd import synth
from rstnet_amd.codec.loaders import get_mimi
from rstnet_amd.lm.model import LMGen, LMModel
from rstnet_amd.pipeline import StreamingPipeline
from tests.helpers import slot_server as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAME = H.FRAME


@functools.lru_cache(maxsize=1)
def _models():
    mimi = get_mimi(synth.mimi_state_dict(H.MIMI_SEED), device=DEV)
    lm = LMModel.from_state_dict({k: v.to(DEV) for k, v in synth.lm_state_dict(H.cfg(), seed=H.LM_SEED).items()}, H.cfg())
    return mimi, lm


def _messages(state_like, fmt: str, wav_row: np.ndarray, token: int):
    msgs = [(S.KIND_AUDIO, S.PcmFramer(FRAME, fmt).encode(wav_row))]
    piece = state_like.text_piece(token)
    if piece is not None:
        msgs.append((S.KIND_TEXT, piece.encode("utf8")))
    return msgs


def _reference(st, row: int, fmt: str, audio: torch.Tensor, neighbour_seed: int):
    """``audio`` fp32 [1, 1, n * FRAME] fed to ``row`` of a new per-stream pipeline from frame 0 -> the messages per frame (the frames
    inside the delay give none).  The other rows get audio no server row ever saw."""
    mimi, lm = _models()
    n = audio.shape[-1] // FRAME
    pcm = synth.synth_audio(H.N, n * FRAME, seed=neighbour_seed)
    pcm[row] = audio[0]
    out = []
    with StreamingPipeline(mimi, LMGen(lm, use_sampling=False), H.N, per_stream=True) as pipe:
        for f in range(n):
            wav = pipe.step(pcm[:, :, f * FRAME:(f + 1) * FRAME].contiguous().to(DEV))
            if wav is None or row not in pipe.stream_valid:
                out.append([])
                continue
            out.append(_messages(st, fmt, wav[row, 0].cpu().numpy(), int(pipe.last_tokens[row, 0])))
    return out


def test_scenario_equals_new_sessions_byte_for_byte():
    mimi, lm = _models()
    st = S.SlotServerState(mimi, lm, DEV, slots=H.N, use_sampling=False)
    try:
        pipe = st.pipe
        st.warmup()
        assert st.ticks == st.max_delay + 3
        fused = (pipe._fused, pipe._fused.graph, pipe._fused.calls)
        assert fused[1] is not None, "the served frame is not one graph after warm-up"
        slot, got = {}, {name: [] for name in H.CLIENTS}
        with torch.no_grad():
            for tick in range(H.TICKS):
                for name, (row, fmt, t0, t1, _, _) in H.CLIENTS.items():
                    if tick == t1 and name in slot:
                        st.leave(slot.pop(name))
                for name, (row, fmt, t0, t1, _, _) in H.CLIENTS.items():
                    if tick == t0:
                        slot[name] = st.join(fmt)
                        assert slot[name] == row, (name, slot[name])
                for name, s in slot.items():
                    p = H.payloads(name)[tick - H.CLIENTS[name][2]]
                    if p is not None:
                        st.push(s, p)
                out = st.tick()
                assert set(out) <= set(slot.values()), "a free row returned something"
                for name, s in slot.items():
                    got[name].append(out.get(s, []))
        assert pipe._fused is fused[0] and pipe._fused.graph is fused[1] and pipe._fused.calls == fused[2], "joins and leaves re-captured the frame"
        assert st.underruns(slot["B"]) == 1 and st.dropped(slot["B"]) == 0 and st.underruns(slot["C"]) == 0
        assert pipe.stream_valid == [0, 1, 2]
    finally:
        st.close()

    d = st.max_delay
    for i, name in enumerate(H.CLIENTS):
        row, fmt, t0, t1, _, _ = H.CLIENTS[name]
        want = _reference(st, row, fmt, H.heard(name), neighbour_seed=70 + i)
        assert len(got[name]) == len(want) == t1 - t0
        assert all(m == [] for m in got[name][:d]) and all(len(m) >= 1 for m in got[name][d:]), name
        for f, (a, b) in enumerate(zip(got[name], want)):
            assert a == b, f"client {name}, frame {f}: {[(k, len(p)) for k, p in a]} against {[(k, len(p)) for k, p in b]}"
        width = 4 if fmt == "f32" else 2
        assert all(m[0][0] == S.KIND_AUDIO and len(m[0][1]) == width * FRAME for m in got[name][d:])
    # not vacuous: had A stayed in row 0 (silence at tick 7, then C's audio, no reset), the row would have said something else than C heard
    a_audio, c_audio = H.heard("A"), H.heard("C")
    stayed = torch.cat([a_audio, torch.zeros(1, 1, FRAME), c_audio], -1)
    tail = _reference(st, 0, "f32", stayed, neighbour_seed=80)[H.CLIENTS["C"][2] + d:]
    assert len(tail) == len(got["C"][d:]) and tail != got["C"][d:]
    assert any(k == S.KIND_TEXT for msgs in got["A"] + got["B"] + got["C"] for k, _ in msgs), "no text piece in the whole scenario"


def test_step_packed_refusals():
    mimi, lm = _models()
    gen = LMGen(lm, use_sampling=False)
    with StreamingPipeline(mimi, gen, 2) as pipe:
        with pytest.raises(ValueError, match="per_stream=True"):
            pipe.step_packed(pipe.new_staged())
        with pytest.raises(ValueError, match="per_stream=True"):
            pipe.set_row_format(0, 0)
    with StreamingPipeline(mimi, gen, 2, per_stream=True) as pipe:
        staged = pipe.new_staged()
        assert tuple(staged.shape) == (2, SL.record_stride(FRAME)) and staged.is_pinned()
        pipe.set_row_format(1, SL.FMT_F32)
        with pytest.raises(ValueError, match="unknown row format"):
            pipe.set_row_format(0, 2)
        with pytest.raises(ValueError, match="outside the batch"):
            pipe.set_row_format(2, 0)
        rec = pipe.step_packed(staged)
        # the eager frames inside everyone's delay: records come back, all invalid
        assert SL.parse_records(rec.numpy(), FRAME) == [None, None] and rec[:, 4:8].view(torch.int32).flatten().tolist() == [-1, -1]
        with pytest.raises(ValueError, match="may not be mixed"):
            pipe.step(torch.zeros(2, 1, FRAME, device=DEV))
        with pytest.raises(ValueError, match="host uint8"):
            pipe.step_packed(staged[:1])
    with StreamingPipeline(mimi, gen, 2, per_stream=True) as pipe:
        pipe.step(torch.zeros(2, 1, FRAME, device=DEV))
        with pytest.raises(ValueError, match="may not be mixed"):
            pipe.step_packed(pipe.new_staged())


@pytest.mark.parametrize("client_rate", [None, 48000], ids=["24k", "48k"])
def test_step_packed_equals_step(client_rate):
    """The packed route adds transport, no arithmetic: the records of ``step_packed`` carry ``PcmFramer.encode`` of what ``step`` returns
    for the same input, frame by frame, through the eager frames and the graph, with and without the two rate conversions in the frame."""
    mimi, lm = _models()
    gen = LMGen(lm, use_sampling=False)
    n_frames, Bp = 6, 2
    names, fmt = ["f32", "s16"], [SL.FMT_F32, SL.FMT_S16]
    want = []
    with StreamingPipeline(mimi, gen, Bp, client_rate=client_rate, per_stream=True) as pipe:
        F = pipe.client_frame
        audio = synth.synth_audio(Bp, n_frames * F, seed=95).numpy()
        sent = [[S.PcmFramer(F, names[b]).encode(audio[b, 0, f * F:(f + 1) * F]) for b in range(Bp)] for f in range(n_frames)]
        heard = [np.stack([_one_frame(F, names[b], sent[f][b]) for b in range(Bp)])[:, None] for f in range(n_frames)]
        for f in range(n_frames):
            wav = pipe.step(torch.from_numpy(heard[f]).to(DEV))
            want.append(None if wav is None else [(int(pipe.last_tokens[b, 0]), S.PcmFramer(F, names[b]).encode(wav[b, 0].cpu().numpy()))
                                                  for b in range(Bp)])
    with StreamingPipeline(mimi, gen, Bp, client_rate=client_rate, per_stream=True) as pipe:
        assert pipe.record_stride == SL.record_stride(F)
        staged = pipe.new_staged()
        for b in range(Bp):
            pipe.set_row_format(b, fmt[b])
        for f in range(n_frames):
            SL.pack_staged(staged.numpy(), sent[f], fmt, F)
            got = SL.parse_records(pipe.step_packed(staged).numpy(), F)
            assert got == (want[f] if want[f] is not None else [None] * Bp), f
        assert pipe._fused is not None and pipe._fused.graph is not None, "the last frames did not run as one graph"
    assert want[0] is None and want[-1] is not None


def _one_frame(F: int, name: str, raw: bytes) -> np.ndarray:
    fr = S.PcmFramer(F, name)
    fr.append_bytes(raw)
    return fr.frames()[0]


def test_websocket_two_clients_at_once_on_the_gpu():
    from aiohttp.test_utils import TestClient, TestServer
    frames = 6
    mimi, lm = _models()

    async def talk(client, query):
        ws = await client.ws_connect("/api/chat" + query)
        assert (await asyncio.wait_for(ws.receive_bytes(), 20.0)) == b"\x00"
        return ws

    async def scenario():
        st = S.SlotServerState(mimi, lm, DEV, slots=2, use_sampling=False)
        st.warmup()
        client = TestClient(TestServer(S.make_app(st)))
        await client.start_server()
        try:
            pcm = synth.synth_audio(2, frames * FRAME, seed=90).numpy()
            raw1 = pcm[0, 0].astype("<f4").tobytes()
            raw2 = (np.clip(pcm[1, 0], -1, 1) * 32767.0).astype("<i2").tobytes()
            ws1, ws2 = await talk(client, ""), await talk(client, "?pcm=s16")
            resp = await client.get("/api/chat")
            assert resp.status == 503
            for ws, raw in ((ws1, raw1), (ws2, raw2)):
                step = len(raw) // 4 + 2                                 # pieces that straddle frame boundaries
                for a in range(0, len(raw), step):
                    await ws.send_bytes(b"\x01" + raw[a:a + step])
            for ws, width in ((ws1, 4), (ws2, 2)):
                audio = []
                while len(audio) < 3:
                    msg = await asyncio.wait_for(ws.receive_bytes(), timeout=20.0)
                    if msg[0] == S.KIND_AUDIO:
                        audio.append(msg[1:])
                assert all(len(p) == width * FRAME for p in audio)
            await ws1.close()
            await ws2.close()
        finally:
            await client.close()
            st.close()

    loop = asyncio.new_event_loop()
    try:
        loop.run_until_complete(scenario())
    finally:
        loop.close()
