"""Band-limited sinc resampling of host waveforms to the codec's 24 kHz -- data preparation in front of the hot path.

The reference hands every waveform whose rate differs from 24 kHz to ``torchaudio.transforms.Resample(sr, 24000)``
(``MLLM_v2/tools/tokenizer/MimiCodec/mimi_tokenizer.py:51-52,66-67``).  torchaudio is a third-party dependency that is neither
vendored under the reference nor installed in this image, so this is a restatement of its published default algorithm
(``torchaudio.functional.resample``: Hann-windowed sinc interpolation, ``lowpass_filter_width=6``, ``rolloff=0.99``; the rates
reduced by their gcd, one polyphase filter per output phase, a strided correlation).  PARITY UNPINNED: no reference test
or fixture holds a resampled waveform and the dependency cannot be run here; the unit tests check the properties that define it
(identity at equal rates, length ``ceil(T * new / orig)``, tone preservation below the cut-off, rejection above it).
Runs on the host (torch CPU) like the reference's call; the codec itself only ever sees 24 kHz.

The second half of the module is the same filter on the device, opt-in: ``resample_device`` (ragged batches, one launch of
``rst_resample_sinc``) and ``StreamResampler`` (live streams, frame by frame, bit-identical to the whole-signal form), both over the
table ``sinc_kernel`` returns.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def sinc_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """-> (filters ``[new, 1, 2 * width + orig]`` fp32, width) for rates already divided by their gcd."""
    base = min(orig_freq, new_freq) * rolloff
    width = math.ceil(lowpass_filter_width * orig_freq / base)
    idx = torch.arange(-width, width + orig_freq, dtype=torch.float64)[None, None] / orig_freq
    t = torch.arange(0, -new_freq, -1, dtype=torch.float64)[:, None, None] / new_freq + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    sinc = torch.where(t == 0, torch.ones_like(t), t.sin() / t)
    return (sinc * window * (base / orig_freq)).float(), width


def resample(wav: torch.Tensor, orig_freq: int, new_freq: int) -> torch.Tensor:
    """``[..., T]`` at ``orig_freq`` -> ``[..., ceil(T * new_freq / orig_freq)]`` at ``new_freq``."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("sample rates must be positive")
    if orig_freq == new_freq:
        return wav
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    kernel, width = sinc_kernel(o, n)
    shape = wav.shape
    x = wav.reshape(-1, shape[-1]).float()
    length = x.shape[1]
    x = F.pad(x, (width, width + o))
    y = F.conv1d(x[:, None], kernel, stride=o).transpose(1, 2).reshape(x.shape[0], -1)
    return y[:, :math.ceil(n * length / o)].reshape(*shape[:-1], -1)


# ---- the same conversion on the device (rst_resample_sinc): ragged batches in front of the codec, and live streams frame by frame ----

_device_tables: dict = {}          # (o, n, device) -> tap-major table, least recently used first
DEVICE_TABLES_MAX = 16
# what a live session may ask for (``stream_pair_geometry``): a client frame of at most 16 codec frames' samples (384 kHz against the
# 24 kHz codec) and tables of at most 2^17 taps x phases (512 KB; the largest of the audio rates, 11.025 <-> 24 kHz, has 51 520)
STREAM_MAX_FRAME_RATIO = 16
STREAM_MAX_TABLE = 1 << 17


def reduce_rates(orig_freq: int, new_freq: int):
    """-> (o, n): the rates divided by their gcd."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("sample rates must be positive")
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def filter_width(o: int, n: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> int:
    """``width`` of ``sinc_kernel(o, n)`` without building the table."""
    return math.ceil(lowpass_filter_width * o / (min(o, n) * rolloff))


def device_table(o: int, n: int, device) -> torch.Tensor:
    """``sinc_kernel(o, n)`` as the library reads it: TAP-MAJOR ``[L, n]`` fp32 on ``device`` (the lanes of a wave hold consecutive
    phases).  Computed in fp64 and rounded once by ``sinc_kernel``, uploaded once per rate pair and device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (o, n, str(device))
    hit = _device_tables.pop(key, None)
    if hit is None:
        kernel, _ = sinc_kernel(o, n)
        hit = kernel[:, 0, :].t().contiguous().to(device)
        while len(_device_tables) >= DEVICE_TABLES_MAX:        # least recently used first (a user that holds a table keeps it alive)
            del _device_tables[next(iter(_device_tables))]
    _device_tables[key] = hit
    return hit


def resample_device(x: torch.Tensor, lengths, orig_freq: int, new_freq: int):
    """Whole signals on the device: ``x [B, T]`` fp32 or int16 (int16 is read as ``v / 32768``), ``lengths [B]`` or ``None`` ->
    ``(y [B, 1, ceil(n * T / o)] fp32, out_lengths [B] int32)`` with ``out_lengths[b] = ceil(n * lengths[b] / o)``.  Row ``b`` equals
    ``resample(x[b, :lengths[b]], orig_freq, new_freq)`` up to fp32 rounding (same table, another summation order) and is exactly
    zero behind ``out_lengths[b]`` -- one launch, no fill.  Equal rates: the int16 -> fp32 conversion and the zero tail only."""
    from .. import ops
    o, n = reduce_rates(orig_freq, new_freq)
    if x.dim() != 2:
        raise ValueError(f"resample_device takes [B, T] rows, got {tuple(x.shape)}")
    B, T = x.shape
    T_out = -(-n * T // o)
    if lengths is None:
        in_len = None
        out_len = torch.full((B,), T_out, dtype=torch.int32, device=x.device)
    else:
        in_len = lengths.to(device=x.device, dtype=torch.int32)
        out_len = torch.div(in_len.to(torch.int64) * n + (o - 1), o, rounding_mode="floor").clamp_(0, T_out).to(torch.int32)
    if o == n:
        y = ops.resample_sinc(x, in_len, None, 1, 1, 0, T_out, out_lengths=out_len)
    else:
        y = ops.resample_sinc(x, in_len, device_table(o, n, x.device), o, n, filter_width(o, n), T_out, out_lengths=out_len)
    return y.unsqueeze(1), out_len


def stream_geometry(orig_freq: int, new_freq: int, frame_out: int):
    """Frame-by-frame conversion that emits ``frame_out`` samples per step -> ``(o, n, width, L, q, hist, frame_in, delay_out)``:
    a step consumes ``frame_in = frame_out * o / n`` samples, keeps the last ``hist = q * o + width`` input samples
    (``q = ceil(width / o)``: the look-ahead ``width`` rounded up to whole input strides) and its output is the whole-signal
    conversion delayed by ``delay_out = q * n`` samples.  ``ValueError`` when ``frame_in`` is not an integer.  Equal rates need
    neither history nor delay (``width = q = hist = delay_out = 0``, ``L = 1``)."""
    o, n = reduce_rates(orig_freq, new_freq)
    frame_out = int(frame_out)
    if frame_out <= 0 or (frame_out * o) % n != 0:
        raise ValueError(f"a frame of {frame_out} samples at {new_freq} Hz is {frame_out * o}/{n} samples at {orig_freq} Hz: not an integer")
    frame_in = frame_out * o // n
    if o == n:
        return 1, 1, 0, 1, 0, 0, frame_in, 0
    width = filter_width(o, n)
    q = -(-width // o)
    return o, n, width, 2 * width + o, q, q * o + width, frame_in, q * n


def stream_pair_geometry(client_rate: int, codec_rate: int, frame_size: int) -> int:
    """Whether a live session can run at ``client_rate`` against a codec of ``frame_size`` samples per frame at ``codec_rate`` ->
    the client's samples per frame.  Host arithmetic only -- no table is built -- so that a server can answer before it commits
    anything.  ``ValueError`` when the frame is not a whole number of client samples, when it is longer than
    ``STREAM_MAX_FRAME_RATIO`` codec frames, when either direction's table ``L * n`` exceeds ``STREAM_MAX_TABLE`` entries, or when
    either direction's history does not fit in front of its chunk (``hist < frame_in``: very low rates)."""
    client_rate, codec_rate, frame_size = int(client_rate), int(codec_rate), int(frame_size)
    if client_rate <= 0:
        raise ValueError("sample rates must be positive")
    if client_rate > STREAM_MAX_FRAME_RATIO * codec_rate:
        raise ValueError(f"{client_rate} Hz is above {STREAM_MAX_FRAME_RATIO} x the codec's {codec_rate} Hz")
    client_frame = stream_geometry(client_rate, codec_rate, frame_size)[6]
    for orig, new, frame_out in ((client_rate, codec_rate, frame_size), (codec_rate, client_rate, client_frame)):
        o, n, _, L, _, hist, frame_in, _ = stream_geometry(orig, new, frame_out)
        if L * n > STREAM_MAX_TABLE:
            raise ValueError(f"{orig} -> {new} Hz needs a filter table of {L} x {n} entries (at most {STREAM_MAX_TABLE} are served)")
        if hist >= frame_in:
            raise ValueError(f"{orig} -> {new} Hz keeps {hist} samples of history, which a frame of {frame_in} samples cannot hold")
    return client_frame


class StreamResampler:
    """``orig_freq -> new_freq`` for ``batch_size`` live streams, ``frame_out`` samples out (``frame_in`` in) per ``step``.  The
    concatenated outputs equal ``concat(zeros(delay_out), resample_device(whole input))`` cut to the emitted length BIT FOR BIT: every
    output is the library's one FMA chain over the same operands, wherever it is computed.  State: one buffer
    ``[B, hist + frame_in]`` (zeroed on construction and by ``reset``).  A step is three stream-ordered operations -- the chunk
    goes behind the history, one ``rst_resample_sinc`` (``lead = 0``) over the buffer into a persistent output, the buffer's last
    ``hist`` samples move to its front (``hist < frame_in``: source and destination do not overlap) -- allocates nothing and can be
    captured in a graph.  ``step`` returns that persistent output: it is valid until the next step.

    The first ``delay_out`` outputs of a session are the filter's response AHEAD of the first sample (outputs at negative time,
    which the whole-signal form never computes): a device-side flag, set by a reset and cleared by the first step after it, masks
    them to +0 (``masked_fill_``: whatever they held, NaN included) -- two small operations that replay unchanged in a graph."""

    def __init__(self, orig_freq: int, new_freq: int, frame_out: int, batch_size: int, device):
        self.orig_freq, self.new_freq, self.batch_size = int(orig_freq), int(new_freq), int(batch_size)
        self.o, self.n, self.width, self.L, self.q, self.hist, self.frame_in, self.delay_out = stream_geometry(orig_freq, new_freq, frame_out)
        self.frame_out = int(frame_out)
        assert self.hist < self.frame_in, (self.hist, self.frame_in)
        device = torch.device(device)
        self.filt = None if self.o == self.n else device_table(self.o, self.n, device)
        self.buf = torch.zeros(self.batch_size, self.hist + self.frame_in, device=device, dtype=torch.float32)
        self.out = torch.zeros(self.batch_size, self.frame_out, device=device, dtype=torch.float32)
        self.fresh = torch.ones(self.batch_size, 1, device=device, dtype=torch.bool)     # per stream: no step since its last reset

    def reset(self) -> None:
        self.buf.zero_()
        self.fresh.fill_(True)

    def reset_rows(self, rows) -> None:
        """Streams ``rows`` start over with the next step (their history zeroed, their first ``delay_out`` outputs masked again); the
        others go on.  In place: a captured step stays valid."""
        rows = sorted({int(r) for r in rows})
        bad = [r for r in rows if not 0 <= r < self.batch_size]
        if bad:
            raise ValueError(f"reset_rows: rows {bad} are outside the batch of {self.batch_size} streams")
        if rows:
            self.buf[rows] = 0.0
            self.fresh[rows] = True

    def step(self, chunk: torch.Tensor) -> torch.Tensor:
        """``chunk [B, 1, frame_in]`` fp32 -> ``[B, 1, frame_out]`` (a view of the persistent output)."""
        from .. import ops
        assert tuple(chunk.shape) == (self.batch_size, 1, self.frame_in), (tuple(chunk.shape), self.frame_in)
        self.buf[:, self.hist:].copy_(chunk[:, 0])
        ops.resample_sinc(self.buf, None, self.filt, self.o, self.n, 0, self.frame_out, out=self.out)
        if self.hist:
            self.buf[:, :self.hist].copy_(self.buf[:, self.frame_in:])
            self.out[:, :self.delay_out].masked_fill_(self.fresh, 0.0)
            self.fresh.fill_(False)
        return self.out.unsqueeze(1)
