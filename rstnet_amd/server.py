"""Full-duplex websocket loop over the streaming path -- the role of ``MLLM_v2/moshi/server.py:44-166``.

Same structure as the reference: one ``ServerState`` holding the codec and ``LMGen`` in ``streaming_forever(1)`` mode, a warm-up of
four silent frames (``:64-73``), one session at a time behind an ``asyncio.Lock`` (``:59,157``), states reset at the start of every
session (``:160-161``), a ``b"\\x00"`` handshake, then per 1920-sample frame ``mimi.encode -> lm_gen.step -> mimi.decode``
(``:122-136``) with audio going out as kind ``1`` messages and text pieces as kind ``2``.

What differs, and why: the reference moves audio as Opus pages through ``sphn`` (``OpusStreamReader`` / ``OpusStreamWriter``);
``sphn`` / libopus are not part of this image, so the transport here is RAW PCM -- the payload of a kind-1 message is
little-endian mono samples at the codec rate, ``f32`` (default) or ``s16`` (``/api/chat?pcm=s16``), in both directions.  The
message kinds, the handshake, the framing and the locking are the reference's; a client only swaps its Opus codec for a
memcpy.  ``/api/chat?pcm=opus`` selects ``OpusFramer`` -- the reference's ``sphn`` reader / writer at the same seam -- which needs the
``sphn`` package and says so when it is missing.  ``/api/chat?sr=<rate>`` (default: the codec's rate) lets a raw-PCM client send and receive
at its own sample rate -- a browser's 48 kHz, telephony's 8 or 16 kHz -- in frames of ``client_geometry`` samples: the two conversions run on the
device (``codec/audio_resample.py``: ``StreamResampler``), which is what the Opus library does for the reference's clients.

``--slots N`` replaces the lock by N rows of one per-stream batch (``SlotServerState`` below): same protocol, N
conversations at once, 503 instead of waiting when all rows are taken, one sample rate per server (``--client-rate``).
``--per-slot-sampling`` (with ``--slots``) lets a client pick its own sampling settings and seed with
``/api/chat?temp=&temp_text=&topk=&topk_text=&seed=&greedy=1`` (``chat_sampling``); without the flag those parameters are refused with 400.
"""
from __future__ import annotations

import asyncio
import time
from typing import Callable, List, Optional

import numpy as np
import torch

KIND_HANDSHAKE, KIND_AUDIO, KIND_TEXT = 0, 1, 2


def log(level: str, msg: str) -> None:
    print(f"[{level}] {msg}", flush=True)


class PcmFramer:
    """Byte stream -> fixed-size frames of float32 samples (the job ``sphn.OpusStreamReader.read_pcm`` + the ``all_pcm_data``
    accumulation of server.py:113-121 do in the reference).  ``fmt``: ``"f32"`` or ``"s16"`` little-endian mono."""

    def __init__(self, frame_size: int, fmt: str = "f32"):
        if fmt not in ("f32", "s16"):
            raise ValueError(f"unknown pcm format {fmt!r}")
        self.frame_size, self.fmt = frame_size, fmt
        self._width = 4 if fmt == "f32" else 2
        self._bytes = bytearray()

    def append_bytes(self, payload: bytes) -> None:
        self._bytes += payload

    def frames(self) -> List[np.ndarray]:
        """All complete frames received so far (a trailing partial frame -- or partial sample -- waits for more bytes)."""
        n = len(self._bytes) // (self._width * self.frame_size)
        out = []
        for i in range(n):
            raw = bytes(self._bytes[i * self._width * self.frame_size:(i + 1) * self._width * self.frame_size])
            out.append(np.frombuffer(raw, dtype="<f4").copy() if self.fmt == "f32"
                       else np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0)
        del self._bytes[:n * self._width * self.frame_size]
        return out

    def encode(self, pcm: np.ndarray) -> bytes:
        """float32 samples -> payload bytes in this framer's format (the outgoing direction)."""
        pcm = np.asarray(pcm, dtype=np.float32).reshape(-1)
        if self.fmt == "f32":
            return pcm.astype("<f4").tobytes()
        return (np.clip(pcm, -1.0, 1.0) * 32767.0).astype("<i2").tobytes()


class OpusFramer:
    """The reference's own transport at the same seam (server.py:105-153): kind-1 payloads are Opus pages, decoded by
    ``sphn.OpusStreamReader`` and re-encoded by ``sphn.OpusStreamWriter``.  ``sphn`` (Rust + libopus) is not part of this image, so
    the class imports it on construction and raises a clear error when it is absent; with it installed, ``/api/chat?pcm=opus``
    speaks the reference client's wire format."""

    def __init__(self, frame_size: int, sample_rate: int):
        try:
            import sphn
        except ImportError as e:
            raise RuntimeError("the Opus transport needs the `sphn` package (absent from this image); use pcm=f32 or pcm=s16") from e
        self.frame_size = frame_size
        self._reader = sphn.OpusStreamReader(sample_rate)
        self._writer = sphn.OpusStreamWriter(sample_rate)
        self._pcm = np.zeros(0, dtype=np.float32)

    def append_bytes(self, payload: bytes) -> None:
        self._reader.append_bytes(payload)

    def frames(self) -> List[np.ndarray]:
        pcm = self._reader.read_pcm()                       # server.py:113-121
        if pcm.shape[-1]:
            self._pcm = np.concatenate((self._pcm, np.asarray(pcm, dtype=np.float32).reshape(-1)))
        n = self._pcm.shape[0] // self.frame_size
        out = [self._pcm[i * self.frame_size:(i + 1) * self.frame_size].copy() for i in range(n)]
        self._pcm = self._pcm[n * self.frame_size:]
        return out

    def encode(self, pcm: np.ndarray) -> bytes:
        """float32 samples -> the Opus bytes that are ready (possibly empty: the writer emits whole pages), server.py:133,146-150."""
        self._writer.append_pcm(np.asarray(pcm, dtype=np.float32).reshape(-1))
        return bytes(self._writer.read_bytes())


def make_framer(frame_size: int, fmt: str, sample_rate: int):
    return OpusFramer(frame_size, sample_rate) if fmt == "opus" else PcmFramer(frame_size, fmt)


def client_geometry(sr: Optional[str], codec_rate: int, frame_size: int):
    """The ``?sr=`` parameter of ``/api/chat`` -> ``(client rate, samples per frame at that rate)``.  Absent or equal to the codec's
    rate: ``(codec_rate, frame_size)``, the plain session.  ``ValueError`` -- answered with 400 before the upgrade -- for a value that is
    not a positive integer, or a rate the stream resamplers do not serve (``audio_resample.stream_pair_geometry``: a codec frame that is
    not a whole number of samples -- refused, not approximated --, a rate so low that the filter's history outgrows a frame, one above
    16 x the codec's, or a ratio whose filter table is out of proportion).  Host arithmetic only: nothing is built or allocated."""
    if sr is None or sr == "":
        return int(codec_rate), int(frame_size)
    try:
        rate = int(sr)
    except ValueError:
        raise ValueError(f"unknown sample rate {sr!r}: ?sr= takes a positive integer (Hz)") from None
    if rate <= 0:
        raise ValueError(f"unknown sample rate {sr!r}: ?sr= takes a positive integer (Hz)")
    if rate == int(codec_rate):
        return rate, int(frame_size)
    from .codec.audio_resample import stream_pair_geometry
    try:
        frame_in = stream_pair_geometry(rate, codec_rate, frame_size)
    except ValueError as e:
        raise ValueError(f"sample rate {rate} cannot be served: {e}") from None
    return rate, frame_in


SAMPLING_QUERY = {"temp": "temp", "temp_text": "temp_text", "topk": "top_k", "topk_text": "top_k_text", "seed": "seed", "greedy": "use_sampling"}


def chat_sampling(query, per_slot_sampling: bool, top_k_cap: int, top_k_text_cap: int) -> Optional[dict]:
    """The sampling parameters of ``/api/chat?temp=&temp_text=&topk=&topk_text=&seed=&greedy=1`` -> the ``sampling`` dict of
    ``SlotServerState.join`` (``set_stream_sampling`` keywords), ``None`` when the client names none.  ``ValueError`` -- answered with 400
    before the upgrade -- when one is present on a server without ``--per-slot-sampling``, for a value that does not parse (a temperature
    is a decimal number, top-k and seed are integers, ``greedy`` is 0 or 1) or lies outside its range (``lm.model.check_sampling``: a
    finite temperature >= 0, a top-k in 1 .. the server's, a seed in 0 .. 2^64 - 1).  ``query``: any mapping of strings (``request.query``).
    Host arithmetic only."""
    from .lm.model import check_sampling
    present = [name for name in SAMPLING_QUERY if query.get(name) not in (None, "")]
    if not present:
        return None
    if not per_slot_sampling:
        raise ValueError(f"this server samples every conversation alike: ?{present[0]}= needs a server started with --slots N --per-slot-sampling")
    out = {}
    for name in present:
        raw, key = query.get(name), SAMPLING_QUERY[name]
        try:
            if name == "greedy":
                if raw not in ("0", "1"):
                    raise ValueError
                out[key] = raw == "0"
            elif name in ("temp", "temp_text"):
                out[key] = float(raw)
            else:
                out[key] = int(raw)
        except ValueError:
            kind = {"greedy": "0 or 1", "temp": "a decimal number", "temp_text": "a decimal number"}.get(name, "an integer")
            raise ValueError(f"?{name}={raw!r} does not parse: it takes {kind}") from None
    try:
        return check_sampling(out, top_k_cap, top_k_text_cap)
    except ValueError as e:
        raise ValueError(f"sampling parameters refused: {e}") from None


class ServerState:
    """``ServerState`` of server.py:44-166 over ``rstnet_amd``'s ``MimiModel`` / ``LMGen`` (or anything with the same three
    calls -- the CPU test drives it with stand-ins)."""

    def __init__(self, mimi, lm, device, text_tokenizer=None, lm_gen=None, **lm_gen_kwargs):
        from .lm.model import LMGen
        self.mimi, self.text_tokenizer, self.device = mimi, text_tokenizer, device
        self.lm_gen = lm_gen if lm_gen is not None else LMGen(lm, **lm_gen_kwargs)
        self.frame_size = int(round(mimi.sample_rate / mimi.frame_rate)) if hasattr(mimi, "frame_rate") else mimi.frame_hop
        self.codec_rate = int(getattr(mimi, "sample_rate", 24000))
        self._session_pair = None        # (client rate, StreamResampler in, StreamResampler out) of the current session's rate: one at a time
        self.lock = asyncio.Lock()
        self.mimi.streaming_forever(1)
        self.lm_gen.streaming_forever(1)

    def _sync(self) -> None:
        if torch.cuda.is_available() and torch.device(self.device).type == "cuda":
            torch.cuda.synchronize(self.device)

    def warmup(self) -> None:
        """server.py:64-73: four silent frames through the whole loop (graph capture happens here, not in the first session)."""
        for _ in range(4):
            chunk = torch.zeros(1, 1, self.frame_size, dtype=torch.float32, device=self.device)
            self.frame(chunk)
        self._sync()

    def rate_pair(self, sr: Optional[int]):
        """The two stream resamplers of a client at ``sr`` Hz (client -> codec, codec -> client), or ``None`` at the codec's own rate."""
        if sr is None or int(sr) == self.codec_rate:
            return None
        if self._session_pair is None or self._session_pair[0] != int(sr):
            from .codec.audio_resample import StreamResampler, stream_pair_geometry
            client_frame = stream_pair_geometry(int(sr), self.codec_rate, self.frame_size)         # ValueError before anything is built
            self._session_pair = None                                                                # (the last rate's buffers go first)
            self._session_pair = (int(sr), StreamResampler(int(sr), self.codec_rate, self.frame_size, 1, self.device),
                                  StreamResampler(self.codec_rate, int(sr), client_frame, 1, self.device))
        return self._session_pair[1:]

    def reset_session(self, sr: Optional[int] = None) -> None:
        """States as a new session finds them (server.py:160-161), the client's two resamplers included."""
        self.mimi.reset_streaming()
        self.lm_gen.reset_streaming()
        pair = self.rate_pair(sr)
        if pair is not None:
            pair[0].reset()
            pair[1].reset()

    def frame(self, chunk: torch.Tensor, sr: Optional[int] = None):
        """One 80 ms frame: pcm ``[1, 1, frame_size]`` -> list of (pcm float32 numpy ``[frame_size]``, text token id) -- empty while
        ``LMGen.step`` still returns ``None`` (the first ``max_delay`` frames), server.py:126-136.  With ``sr`` (a client at another
        rate) the frame comes in and goes out at that rate, ``client_geometry`` samples long."""
        out = []
        pair = self.rate_pair(sr)
        if pair is not None:
            chunk = pair[0].step(chunk)
        codes = self.mimi.encode(chunk)
        for c in range(codes.shape[-1]):
            tokens = self.lm_gen.step(codes[:, :self._n_user(), c:c + 1].contiguous())
            if tokens is None:
                continue
            assert tokens.shape[1] == self.lm_gen.lm_model.dep_q + 1
            main_pcm = self.mimi.decode(tokens[:, 1:].contiguous())
            if pair is not None:
                main_pcm = pair[1].step(main_pcm)
            out.append((main_pcm[0, 0].detach().float().cpu().numpy(), int(tokens[0, 0, 0].item())))
        return out

    def _n_user(self) -> int:
        lm = self.lm_gen.lm_model
        return lm.num_codebooks - lm.dep_q - 1

    def text_piece(self, token: int) -> Optional[str]:
        """server.py:137-142: padding ids 0 / 3 are silent; other ids become sentencepiece pieces (or ``<id>`` without a tokenizer)."""
        if token in (0, 3):
            return None
        if self.text_tokenizer is None:
            return f"<{token}>"
        return self.text_tokenizer.id_to_piece(token).replace("▁", " ")

    async def handle_chat(self, request):
        from aiohttp import WSMsgType, web
        # the transport is settled BEFORE the upgrade: an unknown ?pcm= value, or pcm=opus without `sphn`, is answered with 400 and the
        # reason (after ws.prepare() the client would only see an abrupt 1011 close)
        # so is the client's sample rate (?sr=, default the codec's): PCM comes in and goes out at that rate, in frames of client_frame samples
        try:
            rate, client_frame = client_geometry(request.query.get("sr"), self.codec_rate, self.frame_size)
            framer = make_framer(client_frame, request.query.get("pcm", "f32"), rate)
        except (ValueError, RuntimeError) as e:
            raise web.HTTPBadRequest(text=str(e))
        ws = web.WebSocketResponse()
        await ws.prepare(request)
        close = False
        outbox: asyncio.Queue = asyncio.Queue()

        async def recv_loop():
            nonlocal close
            try:
                async for message in ws:
                    if message.type == WSMsgType.ERROR:
                        log("error", f"{ws.exception()}")
                        break
                    if message.type in (WSMsgType.CLOSED, WSMsgType.CLOSE):
                        break
                    if message.type != WSMsgType.BINARY:
                        log("error", f"unexpected message type {message.type}")
                        continue
                    data = message.data
                    if len(data) == 0:
                        log("warning", "empty message")
                        continue
                    if data[0] == KIND_AUDIO:
                        framer.append_bytes(data[1:])
                    else:
                        log("warning", f"unknown message kind {data[0]}")
            finally:
                close = True
                log("info", "connection closed")

        async def frame_loop():
            while not close:
                await asyncio.sleep(0.001)
                for pcm in framer.frames():
                    be = time.time()
                    chunk = torch.from_numpy(pcm).to(self.device)[None, None]
                    for out_pcm, text_token in self.frame(chunk, rate):
                        payload = framer.encode(out_pcm)
                        if len(payload) > 0:            # (an Opus writer hands out whole pages: nothing yet is not a message)
                            await outbox.put(bytes([KIND_AUDIO]) + payload)
                        piece = self.text_piece(text_token)
                        if piece is not None:
                            await outbox.put(bytes([KIND_TEXT]) + piece.encode("utf8"))
                    log("info", f"frame handled in {1000 * (time.time() - be):.1f}ms")

        async def send_loop():
            while not close or not outbox.empty():
                try:
                    msg = await asyncio.wait_for(outbox.get(), timeout=0.005)
                except asyncio.TimeoutError:
                    continue
                try:
                    await ws.send_bytes(msg)
                except (ConnectionError, RuntimeError):
                    return

        log("info", "accepted connection")
        async with self.lock:       # one session at a time (server.py:157)
            self.reset_session(rate)
            await ws.send_bytes(bytes([KIND_HANDSHAKE]))
            await asyncio.gather(frame_loop(), recv_loop(), send_loop())
        log("info", "done with connection")
        return ws


class SlotServerState:
    """``--slots N``: N conversations at once, each in one row of ONE ``StreamingPipeline(per_stream=True)`` of batch N that is entered
    once and lives as long as the server.  A fixed clock runs one frame per codec frame period (sooner when every
    occupied row already has its frame): ``tick`` applies the joins since the last tick in one ``reset_streams``, packs one record per
    row from the inboxes, runs ``step_packed`` -- one upload, one graph replay, one download -- and turns the valid records into the
    kind-1 / kind-2 messages of their slots.  A row without a frame at a tick is fed silence and counted (``underruns``); it is not
    waited for.

    Every GPU call is issued by ``tick`` (and ``warmup``), and ``tick`` runs on the event loop's own thread: ``join`` / ``push`` /
    ``leave`` only touch host tables.  A frame blocks the loop for the ~8 ms of its graph out of an 80 ms period, in which nothing but
    socket reads and writes would run; in exchange there is no second thread whose current stream, device guard or capture state could
    differ from the one the graph was captured under, and the tables need no lock.

    The driver API (``join`` / ``push`` / ``leave`` / ``tick``) works without sockets; ``handle_chat`` is a thin layer over it.
    ``pipeline=``: anything with the pipeline's packed surface (the CPU tests pass a stand-in)."""

    def __init__(self, mimi, lm, device, slots: int, client_rate: Optional[int] = None, text_tokenizer=None, lm_gen=None, pipeline=None,
                 max_backlog: int = 4, per_slot_sampling: bool = False, **lm_gen_kwargs):
        from . import slots as SL
        if not 1 <= int(slots) <= 64:
            raise ValueError(f"--slots takes 1 .. 64 rows, got {slots}")
        self.SL, self.mimi, self.text_tokenizer, self.device, self.n = SL, mimi, text_tokenizer, device, int(slots)
        self.codec_rate = int(getattr(mimi, "sample_rate", 24000))
        self.frame_size = int(round(mimi.sample_rate / mimi.frame_rate)) if hasattr(mimi, "frame_rate") else mimi.frame_hop
        self.period = self.frame_size / float(self.codec_rate)           # seconds per frame, from the codec (80 ms for Mimi)
        self.client_rate = self.codec_rate if client_rate is None else int(client_rate)
        if pipeline is None:
            from .lm.model import LMGen
            from .pipeline import StreamingPipeline
            # --per-slot-sampling: every row samples by its own device-table entries, set from its client's query
            lm_gen = lm_gen if lm_gen is not None else LMGen(lm, **dict(lm_gen_kwargs, **({"per_stream_sampling": True} if per_slot_sampling else {})))
            pipeline = StreamingPipeline(mimi, lm_gen, self.n, client_rate=None if self.client_rate == self.codec_rate else self.client_rate,
                                         per_stream=True)
            pipeline.__enter__()                                           # once: the session is the server's lifetime
        self.pipe = pipeline
        self.max_delay = int(self.pipe.lm_gen.max_delay)
        self.F = int(self.pipe.client_frame)
        self.table = SL.SlotTable(self.n)
        self.max_backlog = int(max_backlog)
        self.fmt: List[int] = [SL.FMT_FREE] * self.n                       # host mirror of the pipeline's fmt vector
        self.inbox: List[Optional[object]] = [None] * self.n
        self._freed: List[int] = []                                        # rows left since the last tick (their fmt word goes to -1 there)
        self.per_slot_sampling = bool(per_slot_sampling)
        self._sampling: dict = {}                                          # joining slot -> its client's sampling settings (applied at the tick)
        self._custom: set = set()                                          # rows whose tables hold a client's settings, not the server's defaults
        self._on_live: dict = {}                                           # slot -> asyncio.Event set when its reset has been applied
        self._outbox: dict = {}                                            # slot -> asyncio.Queue of (kind, payload)
        self._staged = self.pipe.new_staged()
        self._staged_np = self._staged.numpy()
        self.ticks = 0
        self._clock_task = None

    def close(self) -> None:
        """Ends the pipeline's session (its states and the captured frame are released).  The server process never needs to."""
        self.pipe.__exit__(None, None, None)

    # ---- driver API ----------------------------------------------------------------------------------------------------------------

    def sampling_caps(self):
        """``(top_k, top_k_text)`` of the served ``LMGen``: the caps of a client's own values."""
        d = self.pipe.lm_gen.default_sampling()
        return max(int(d["top_k"]), 1), max(int(d["top_k_text"]), 1)

    def join(self, fmt: str, sampling: Optional[dict] = None) -> Optional[int]:
        """Claims the lowest free row for a client whose transport is ``fmt`` (``"f32"`` / ``"s16"``); ``None`` when all are taken.  The
        row starts its conversation at the next tick.  ``sampling``: the client's own settings, ``set_stream_sampling`` keywords
        (validated here, ``ValueError``; applied at that tick, over the server's defaults); ``None``: the server's defaults and a new seed."""
        SL = self.SL
        if fmt not in SL.FMT_CODES:
            raise ValueError(f"unknown pcm format {fmt!r}")
        if sampling is not None:
            from .lm.model import check_sampling
            sampling = check_sampling(sampling, *self.sampling_caps())
        slot = self.table.acquire()
        if slot is None:
            return None
        if sampling is not None:
            self._sampling[slot] = sampling
        self.fmt[slot] = SL.FMT_CODES[fmt]
        self.inbox[slot] = SL.Inbox(self.F * SL.sample_width(self.fmt[slot]), self.max_backlog)
        return slot

    def push(self, slot: int, payload: bytes) -> None:
        """Incoming audio bytes of ``slot`` in its transport (any split; whole frames queue up, the oldest beyond ``max_backlog`` is dropped)."""
        if self.table.state(slot) == self.SL.FREE:
            raise ValueError(f"slot {slot} is free")
        self.inbox[slot].push(payload)

    def leave(self, slot: int) -> None:
        """Frees the row.  It goes on computing (on silence) without anything being returned; it is reset when it is next acquired."""
        self.table.release(slot)
        self._sampling.pop(slot, None)
        self.fmt[slot] = self.SL.FMT_FREE
        self._freed.append(slot)
        self._on_live.pop(slot, None)
        self._outbox.pop(slot, None)

    def underruns(self, slot: int) -> int:
        return self.inbox[slot].underruns

    def dropped(self, slot: int) -> int:
        return self.inbox[slot].dropped

    def tick(self) -> dict:
        """One frame for every row -> ``{slot: [(kind, payload bytes), ...]}`` for the rows that produced output."""
        SL = self.SL
        for b in self._freed:
            if self.table.state(b) == SL.FREE:
                self.pipe.set_row_format(b, SL.FMT_FREE)
        self._freed = []
        joined = self.table.rows(SL.JOINING)
        if joined:
            self.pipe.reset_streams(joined)                # ONE call for all of them: a reset's host cost does not grow with the row count
            self._apply_sampling(joined)
            for b in joined:
                self.pipe.set_row_format(b, self.fmt[b])
                self.table.mark_live(b)
        frames: List[Optional[bytes]] = [None] * self.n
        for b in self.table.rows(SL.LIVE):
            frames[b] = self.inbox[b].pop()
            if frames[b] is None and b not in joined:      # (the tick that applies a join precedes the handshake: no frame is owed yet)
                self.inbox[b].underruns += 1
        SL.pack_staged(self._staged_np, frames, self.fmt, self.F)
        records = self.pipe.step_packed(self._staged)
        self.ticks += 1
        out: dict = {}
        live = set(self.table.rows(SL.LIVE))
        for b, rec in enumerate(SL.parse_records(records.numpy(), self.F)):
            if rec is None or b not in live:
                continue
            token, payload = rec
            msgs = [(KIND_AUDIO, payload)]
            piece = self.text_piece(token)
            if piece is not None:
                msgs.append((KIND_TEXT, piece.encode("utf8")))
            out[b] = msgs
        for b in joined:
            ev = self._on_live.get(b)
            if ev is not None:
                ev.set()
        return out

    def _apply_sampling(self, joined: List[int]) -> None:
        """The sampling settings of the rows that just joined, after their reset (which drew each a new seed): a client's own over the
        server's defaults; the defaults again for a row whose previous client had its own.  One call for all of them (per-row value
        lists: one table write per field, not per row) and one for the seeds that clients named.  Rows that never held a client's
        settings are not touched -- a pipeline without ``set_stream_sampling`` serves any number of joins without ``sampling``."""
        settings = {b: self._sampling.pop(b, None) for b in joined}
        rows = [b for b in joined if settings[b] is not None or b in self._custom]
        if not rows:
            return
        defaults = self.pipe.lm_gen.default_sampling()
        full = [dict(defaults, **{k: v for k, v in (settings[b] or {}).items() if k != "seed"}) for b in rows]
        self.pipe.set_stream_sampling(rows, **{k: [f[k] for f in full] for k in defaults})
        seeded = [b for b in rows if settings[b] is not None and "seed" in settings[b]]
        if seeded:
            self.pipe.set_stream_sampling(seeded, seed=[settings[b]["seed"] for b in seeded])
        self._custom = (self._custom - set(rows)) | {b for b in rows if settings[b] is not None}

    text_piece = ServerState.text_piece

    def warmup(self) -> None:
        """``max_delay + 3`` silent frames with every row free: the modules' eager frames, then the capture -- before the first client."""
        with torch.no_grad():
            for _ in range(self.max_delay + 3):
                self.tick()
        fused = getattr(self.pipe, "_fused", None)
        wants_graph = getattr(self.pipe, "fuse", False) and torch.device(self.device).type == "cuda"
        if wants_graph and not (fused is not None and fused.disable):
            assert fused is not None and fused.graph is not None, "the served frame was not captured during warm-up"

    # ---- sockets -------------------------------------------------------------------------------------------------------------------

    async def clock(self) -> None:
        """The one place frames are run from: polls the inboxes and runs ``tick`` when ``slots.tick_due`` says so."""
        SL = self.SL
        loop = asyncio.get_running_loop()
        last = loop.time()
        while True:
            await asyncio.sleep(0.002)
            occupied = self.table.occupied()
            # a joining row waits for nothing but its reset: it counts as ready
            ready = [b for b in occupied if self.table.state(b) == SL.JOINING or len(self.inbox[b]) > 0]
            now = loop.time()
            if not SL.tick_due(ready, occupied, now - last, self.period):
                if not occupied:
                    last = now
                continue
            last = now
            with torch.no_grad():
                msgs = self.tick()
            for slot, items in msgs.items():
                q = self._outbox.get(slot)
                if q is not None:
                    for item in items:
                        q.put_nowait(item)

    async def start_clock(self, app=None) -> None:
        self._clock_task = asyncio.get_running_loop().create_task(self.clock())

    async def stop_clock(self, app=None) -> None:
        if self._clock_task is not None:
            self._clock_task.cancel()
            try:
                await self._clock_task
            except asyncio.CancelledError:
                pass
            self._clock_task = None

    async def handle_chat(self, request):
        from aiohttp import WSMsgType, web
        # everything that can refuse a client is settled BEFORE the upgrade: transport and rate (400), a free row (503)
        try:
            rate, client_frame = client_geometry(request.query.get("sr"), self.codec_rate, self.frame_size)
            if rate != self.client_rate:
                raise ValueError(f"this server serves clients at {self.client_rate} Hz (--client-rate); ?sr={rate} is another rate")
            kind = request.query.get("pcm", "f32")
            framer = make_framer(self.F, kind, rate) if kind == "opus" else None
            if kind != "opus" and kind not in self.SL.FMT_CODES:
                raise ValueError(f"unknown pcm format {kind!r}")
            sampling = chat_sampling(request.query, self.per_slot_sampling, *(self.sampling_caps() if self.per_slot_sampling else (1, 1)))
        except (ValueError, RuntimeError) as e:
            raise web.HTTPBadRequest(text=str(e))
        slot = self.join("f32" if framer is not None else kind, sampling)        # an Opus client's row runs as f32 behind its own host framer
        if slot is None:
            raise web.HTTPServiceUnavailable(text=f"all {self.n} slots are taken; try again when a conversation has ended")
        live, outbox = asyncio.Event(), asyncio.Queue()
        self._on_live[slot], self._outbox[slot] = live, outbox
        close = False
        try:
            ws = web.WebSocketResponse()
            await ws.prepare(request)

            async def recv_loop():
                nonlocal close
                try:
                    async for message in ws:
                        if message.type == WSMsgType.ERROR:
                            log("error", f"{ws.exception()}")
                            break
                        if message.type in (WSMsgType.CLOSED, WSMsgType.CLOSE):
                            break
                        if message.type != WSMsgType.BINARY:
                            log("error", f"unexpected message type {message.type}")
                            continue
                        data = message.data
                        if len(data) == 0:
                            log("warning", "empty message")
                            continue
                        if data[0] != KIND_AUDIO:
                            log("warning", f"unknown message kind {data[0]}")
                        elif framer is None:
                            self.push(slot, data[1:])
                        else:
                            framer.append_bytes(data[1:])
                            for pcm in framer.frames():
                                self.push(slot, np.asarray(pcm, dtype="<f4").tobytes())
                finally:
                    close = True
                    log("info", f"slot {slot}: connection closed")

            async def send_loop():
                while not close or not outbox.empty():
                    try:
                        kind_out, payload = await asyncio.wait_for(outbox.get(), timeout=0.005)
                    except asyncio.TimeoutError:
                        continue
                    if framer is not None and kind_out == KIND_AUDIO:
                        payload = framer.encode(np.frombuffer(payload, dtype="<f4"))
                        if len(payload) == 0:           # (an Opus writer hands out whole pages: nothing yet is not a message)
                            continue
                    try:
                        await ws.send_bytes(bytes([kind_out]) + payload)
                    except (ConnectionError, RuntimeError):
                        return

            log("info", f"slot {slot}: accepted connection")
            await live.wait()                           # the row's reset has been applied: the conversation starts with the next frame
            await ws.send_bytes(bytes([KIND_HANDSHAKE]))
            await asyncio.gather(recv_loop(), send_loop())
        finally:
            self.leave(slot)
        log("info", f"slot {slot}: done with connection")
        return ws


def make_app(state):
    from aiohttp import web
    app = web.Application()
    app.router.add_get("/api/chat", state.handle_chat)
    if isinstance(state, SlotServerState):
        app.on_startup.append(state.start_clock)
        app.on_cleanup.append(state.stop_clock)
    return app


def make_state(mimi, lm, device, args, text_tokenizer=None):
    """``ServerState`` (one session behind a lock, the reference's loop) unless ``--slots N`` asks for the slot server."""
    slots = getattr(args, "slots", None)
    if slots is None:
        return ServerState(mimi, lm, device, text_tokenizer=text_tokenizer)
    return SlotServerState(mimi, lm, device, slots=slots, client_rate=getattr(args, "client_rate", None), text_tokenizer=text_tokenizer,
                           per_slot_sampling=bool(getattr(args, "per_slot_sampling", False)))


def build_state(args, log_fn: Callable[[str, str], None] = log):
    """Models for the CLI: checkpoints (``--mimi-weight`` / ``--moshi-weight``, safetensors or torch files) or ``--synthetic``
    seeded random-init weights of the real shapes (there is no hub access in this image)."""
    from . import synth
    from .codec.loaders import get_mimi
    from .lm.model import LMModel
    device = torch.device(args.device)
    if device.type == "cuda":
        if device.index is None:         # the default `--device cuda`: set_device wants an index
            device = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(device)
    cfg = dict(synth.LM_MOSHI_7B if args.lm_config == "moshi7b" else synth.LM_TINY_16Q)
    if args.synthetic:
        mimi = get_mimi(synth.mimi_state_dict(0), device=device)
        sd = synth.lm_state_dict(cfg, seed=0, device=str(device))
    else:
        from .lm.loaders import load_lm_state_dict
        mimi = get_mimi(args.mimi_weight, device=device)
        sd = load_lm_state_dict(args.moshi_weight, device=device)
    lm = LMModel.from_state_dict(sd, cfg, weight_dtype=getattr(args, "lm_weights", "bf16"),
                                 batched=getattr(args, "lm_mxfp4_batched", False))
    tok = None
    if args.tokenizer:
        import sentencepiece
        tok = sentencepiece.SentencePieceProcessor(args.tokenizer)
    log_fn("info", "models loaded")
    return make_state(mimi, lm, device, args, text_tokenizer=tok)


def main(argv=None) -> None:
    import argparse
    from aiohttp import web
    p = argparse.ArgumentParser(description="raw-PCM websocket server over the MI355X streaming path (moshi/server.py without Opus)")
    p.add_argument("--host", default="localhost", type=str)
    p.add_argument("--port", default=8998, type=int)
    p.add_argument("--tokenizer", type=str, help="path to a local sentencepiece model (text pieces; ids are sent as <id> without it)")
    p.add_argument("--moshi-weight", type=str, help="path to a local checkpoint file for the LM")
    p.add_argument("--mimi-weight", type=str, help="path to a local checkpoint file for Mimi")
    p.add_argument("--synthetic", action="store_true", help="seeded random-init weights of the real shapes (no checkpoints needed)")
    p.add_argument("--lm-config", choices=["moshi7b", "tiny"], default="moshi7b")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--lm-weights", choices=["bf16", "fp8", "mxfp4"], default="bf16",
                   help="storage of the LM's streamed weights: fp8 = e4m3 weight-only copies (GEMV at one or two streams, fp8 skinny GEMM above), mxfp4 = OCP MXFP4 copies "
                        "of the temporal stack's per-layer matrices with the heads at fp8 (LMModel.quantize_weights_; speech quality "
                        "under fp8 or mxfp4 weights has not been evaluated)")
    p.add_argument("--lm-mxfp4-batched", action="store_true",
                   help="with --lm-weights mxfp4: stream the MXFP4 copies above two streams too (weight-only MXFP4 skinny GEMM) instead of "
                        "reading those matrices as bf16 there; same values, a quarter of the bytes, no packed bf16 copies (opt-in)")
    p.add_argument("--slots", type=int, default=None,
                   help="serve up to N conversations at once (1 .. 64), each in one row of a per-stream batch of N behind one frame graph; a "
                        "client beyond N is refused with 503.  Without it: one session at a time behind a lock, as the reference serves")
    p.add_argument("--client-rate", type=int, default=None,
                   help="with --slots: the one sample rate of every raw-PCM client (default: the codec's); another ?sr= is refused with 400")
    p.add_argument("--per-slot-sampling", action="store_true",
                   help="with --slots: every conversation samples by its own settings and noise stream, set by its client with "
                        "?temp=&temp_text=&topk=&topk_text=&seed=&greedy=1 (top-k up to the server's values); without it those parameters are refused with 400")
    args = p.parse_args(argv)
    if args.per_slot_sampling and args.slots is None:
        p.error("--per-slot-sampling needs --slots")
    if args.slots is not None and not 1 <= args.slots <= 64:
        p.error("--slots takes 1 .. 64")
    if args.client_rate is not None and args.slots is None:
        p.error("--client-rate needs --slots (without it every client names its own rate with ?sr=)")
    if args.lm_mxfp4_batched and args.lm_weights != "mxfp4":
        p.error("--lm-mxfp4-batched needs --lm-weights mxfp4")
    if not args.synthetic and not (args.moshi_weight and args.mimi_weight):
        p.error("give --moshi-weight and --mimi-weight, or --synthetic")
    torch.manual_seed(42424242)
    state = build_state(args)
    log("info", "warming up the model")
    state.warmup()
    log("info", f"Access the websocket at ws://{args.host}:{args.port}/api/chat  (raw PCM payloads; Opus needs sphn, absent here)")
    with torch.no_grad():
        web.run_app(make_app(state), host=args.host, port=args.port)


if __name__ == "__main__":
    main()
