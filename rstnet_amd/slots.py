"""Host side of serving N conversations over one per-stream frame graph: which row of the batch a client owns, when a
frame runs, what waits for it, and the two record layouts that carry a whole batch in one upload and one download per frame
(``rst_frame_ingress`` / ``rst_frame_egress``, include/rstnet_hip.h).  numpy only: nothing here needs a GPU, the library or torch.

A record buffer is uint8 ``[B, REC]``, ``REC = record_stride(F) = round_up(16 + 4 F, 16)``, little-endian:

  ingress record   int32 present | 12 reserved bytes | F samples, f32 or s16 as the row's format says
  egress record    int32 valid | int32 text token (-1 when not valid) | int32 payload bytes | int32 0 | payload | zeros up to REC
"""
from __future__ import annotations

from collections import deque
from typing import Deque, Dict, List, Optional, Sequence, Tuple

import numpy as np

FMT_FREE, FMT_F32, FMT_S16 = -1, 0, 1
FMT_CODES = {"f32": FMT_F32, "s16": FMT_S16}
FMT_NAMES = {v: k for k, v in FMT_CODES.items()}
HEADER = 16
FREE, JOINING, LIVE = "free", "joining", "live"


def record_stride(F: int) -> int:
    """Bytes between two records of ``F``-sample frames.  The 16-byte rounding matters for a frame length that is no multiple of four
    (882 samples at 11.025 kHz): without it every second row would start off a 16-byte boundary."""
    return (HEADER + 4 * int(F) + 15) // 16 * 16


def sample_width(fmt: int) -> int:
    return 2 if fmt == FMT_S16 else 4


class SlotTable:
    """Rows of the batch as slots.  FREE -> ``acquire()`` -> JOINING (claimed; its reset has not been applied yet) -> ``mark_live`` ->
    LIVE -> ``release`` -> FREE.  ``acquire`` hands out the lowest free row."""

    def __init__(self, n: int):
        if n < 1:
            raise ValueError(f"a slot table needs at least one row, got {n}")
        self.n = int(n)
        self._state: List[str] = [FREE] * self.n

    def acquire(self) -> Optional[int]:
        for b, s in enumerate(self._state):
            if s == FREE:
                self._state[b] = JOINING
                return b
        return None

    def mark_live(self, b: int) -> None:
        if self._state[b] != JOINING:
            raise ValueError(f"row {b} is {self._state[b]}, not joining")
        self._state[b] = LIVE

    def release(self, b: int) -> None:
        if not 0 <= b < self.n or self._state[b] == FREE:
            raise ValueError(f"row {b} is not held")
        self._state[b] = FREE

    def state(self, b: int) -> str:
        return self._state[b]

    def rows(self, state: str) -> List[int]:
        return [b for b, s in enumerate(self._state) if s == state]

    def occupied(self) -> List[int]:
        return [b for b, s in enumerate(self._state) if s != FREE]


def tick_due(ready: Sequence[int], occupied: Sequence[int], elapsed: float, period: float) -> bool:
    """Whether a frame runs now.  Never without an occupied row; otherwise as soon as every occupied row has a frame queued (``ready``),
    or when the frame period has passed since the last tick, whoever is late.  A fixed clock: a late row is fed silence, not waited for."""
    if not occupied:
        return False
    if set(occupied) <= set(ready):
        return True
    return elapsed >= period


class Inbox:
    """The frames of one row waiting for their tick, oldest first, at most ``max_backlog`` of them: a client that runs ahead loses its
    OLDEST frame (the conversation stays close to real time) and ``dropped`` counts it."""

    def __init__(self, frame_bytes: int, max_backlog: int = 4):
        if max_backlog < 1:
            raise ValueError("max_backlog must be at least 1")
        self.frame_bytes, self.max_backlog = int(frame_bytes), int(max_backlog)
        self._partial = bytearray()
        self._frames: Deque[bytes] = deque()
        self.dropped = 0
        self.underruns = 0

    def push(self, payload: bytes) -> None:
        """Bytes as they arrive (message boundaries need not be frame boundaries); whole frames move to the queue."""
        self._partial += payload
        n = len(self._partial) // self.frame_bytes
        for i in range(n):
            self._frames.append(bytes(self._partial[i * self.frame_bytes:(i + 1) * self.frame_bytes]))
        del self._partial[:n * self.frame_bytes]
        while len(self._frames) > self.max_backlog:
            self._frames.popleft()
            self.dropped += 1

    def pop(self) -> Optional[bytes]:
        return self._frames.popleft() if self._frames else None

    def __len__(self) -> int:
        return len(self._frames)


def pack_staged(buf: np.ndarray, frames: Sequence[Optional[bytes]], fmt: Sequence[int], F: int) -> None:
    """Fills the ingress buffer ``buf`` (uint8 ``[B, REC]``) in place: row ``b`` gets ``present = 1`` and the payload bytes ``frames[b]``
    (``F`` samples in the row's transport), or ``present = 0`` for ``None`` (the payload of such a row is not read)."""
    B, REC = buf.shape
    assert REC >= record_stride(F) and len(frames) == B and len(fmt) == B
    head = buf[:, :4].view("<i4")
    for b, fr in enumerate(frames):
        if fr is None:
            head[b, 0] = 0
            continue
        n = F * sample_width(fmt[b])
        if len(fr) != n:
            raise ValueError(f"row {b}: a frame of {F} {FMT_NAMES.get(fmt[b], fmt[b])} samples is {n} bytes, got {len(fr)}")
        head[b, 0] = 1
        buf[b, HEADER:HEADER + n] = np.frombuffer(fr, dtype=np.uint8)


def parse_records(buf: np.ndarray, F: int) -> List[Optional[Tuple[int, bytes]]]:
    """Egress buffer uint8 ``[B, REC]`` -> per row ``None`` (not valid) or ``(text token, payload bytes)``."""
    B, REC = buf.shape
    assert REC >= record_stride(F)
    head = buf[:, :HEADER].view("<i4")
    out: List[Optional[Tuple[int, bytes]]] = []
    for b in range(B):
        if head[b, 0] == 0:
            out.append(None)
            continue
        n = int(head[b, 2])
        assert 0 <= n <= REC - HEADER, (b, n)
        out.append((int(head[b, 1]), buf[b, HEADER:HEADER + n].tobytes()))
    return out


def egress_reference(wav: np.ndarray, tokens: np.ndarray, offsets: Sequence[int], max_delay: int, fmt: Sequence[int], F: int) -> np.ndarray:
    """The egress record buffer in numpy: what ``rst_frame_egress`` must write, byte for byte.  ``wav`` fp32 ``[B, 1, F]`` (or ``[B, F]``),
    ``tokens`` int64 ``[B, 1 + dep_q]``, ``offsets`` the per-stream frame counters after the commit.  The payload of a valid row is
    ``PcmFramer.encode`` of its samples in its format; NaN, whose s16 conversion numpy leaves undefined, is defined as 0."""
    from .server import PcmFramer
    wav = np.asarray(wav, dtype=np.float32).reshape(len(fmt), -1)
    B = wav.shape[0]
    assert wav.shape[1] == F
    buf = np.zeros((B, record_stride(F)), dtype=np.uint8)
    head = buf[:, :HEADER].view("<i4")
    for b in range(B):
        if not (fmt[b] >= 0 and int(offsets[b]) > max_delay):
            head[b, 1] = -1
            continue
        name = "s16" if fmt[b] == FMT_S16 else "f32"
        row = wav[b]
        if name == "s16":
            row = np.where(np.isnan(row), np.float32(0.0), row)
        payload = PcmFramer(F, name).encode(row)
        head[b, 0], head[b, 1], head[b, 2] = 1, int(tokens[b][0]), len(payload)
        buf[b, HEADER:HEADER + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    return buf


def ingress_reference(buf: np.ndarray, fmt: Sequence[int], F: int) -> np.ndarray:
    """The ingress in numpy: records -> fp32 ``[B, 1, F]``; the s16 formula is ``PcmFramer.frames``'."""
    B = buf.shape[0]
    out = np.zeros((B, 1, F), dtype=np.float32)
    head = buf[:, :4].view("<i4")
    for b in range(B):
        if head[b, 0] == 0 or fmt[b] < 0:
            continue
        raw = buf[b, HEADER:HEADER + F * sample_width(fmt[b])].tobytes()
        out[b, 0] = (np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0) if fmt[b] == FMT_S16 else np.frombuffer(raw, dtype="<f4")
    return out
