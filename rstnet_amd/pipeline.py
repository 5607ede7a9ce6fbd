"""End-to-end streaming loop: PCM in -> Mimi encode -> LMGen.step -> Mimi decode -> PCM out, one 80 ms frame per call.

This is the loop of the reference's ``MLLM_v2/moshi/server.py:122-136`` (``opus_loop``) without the Opus / websocket
transport: ``mimi.encode(chunk)`` -> ``lm_gen.step(codes)`` -> ``mimi.decode(tokens[:, 1:])``; the first ``max_delay``
frames produce no output (``LMGen.step`` returns ``None``).  All state (conv histories, KV rings, token ring
cache) lives in the modules' streaming states on the device; the host only moves 1920 samples in and out per stream.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from .codec.audio_resample import StreamResampler, stream_pair_geometry
from .codec.mimi import MimiCodec
from .codec.streaming import check_rows
from .graphs import Graphed, RecaptureGate
from .lm.model import LMGen
from .slots import record_stride

CODEC_RATE = 24000


def restart_schedule(frames: Sequence[int], awaiting: Sequence[int], max_delay: int) -> Tuple[List[int], List[int], List[int]]:
    """The host side of one frame of a per-stream session, as a pure function.  ``frames[b]``: frames stream ``b`` has stepped since its
    (re)start, BEFORE this frame; ``awaiting``: the restarted streams whose decoder side still has to be reset a second time.  ->
    ``(reset_now, valid, awaiting_after)``:

    * ``reset_now``: streams of ``awaiting`` whose decoder side is reset immediately before this frame -- the frame that produces their
      first valid output (``frames[b] == max_delay``).  A new session does not run the decoder or the outgoing rate conversion during its
      first ``max_delay`` frames; in a batch both run for every stream on every frame, so whatever a restarted stream's delay frames
      left in its decoder state is wiped here.
    * ``valid``: streams whose output of this frame is meaningful, ``frames[b] + 1 > max_delay``; the others' PCM is zero-filled.
    * ``awaiting_after``: ``awaiting`` without ``reset_now``."""
    reset_now = sorted(b for b in set(awaiting) if frames[b] == max_delay)
    valid = [b for b, n in enumerate(frames) if n + 1 > max_delay]
    return reset_now, valid, sorted(set(awaiting) - set(reset_now))


class StreamingPipeline:
    def __init__(self, mimi: MimiCodec, lm_gen: LMGen, batch_size: int, client_rate: Optional[int] = None, per_stream: bool = False):
        assert mimi.quantizer.n_q >= lm_gen.lm_model.dep_q
        self.mimi, self.lm_gen, self.batch_size = mimi, lm_gen, batch_size
        # per_stream: every stateful module of the frame keeps one position per stream, so `reset_streams(rows)` can start new conversations
        # in single rows of the live batch while the others go on; `step` then returns PCM for all rows (zeros for rows inside their delay)
        self.per_stream = bool(per_stream)
        self._frames: List[int] = [0] * batch_size      # per-stream: frames each row has stepped since its (re)start
        self._awaiting: List[int] = []                  # per-stream: restarted rows whose decoder side is reset once more (restart_schedule)
        self.stream_valid: List[int] = []               # rows whose PCM of the last `step` is meaningful
        self.frame_size = mimi.frame_hop
        # a client at another sample rate: ``step`` takes and returns ``client_frame`` samples at ``client_rate``; the two conversions
        # (codec/audio_resample.py: StreamResampler, created per session) are part of the frame.  ValueError here, before any streaming
        # context is entered, for a rate the resamplers do not serve (stream_pair_geometry: no whole-sample frame, too low, too high)
        self.client_rate = None if client_rate is None else int(client_rate)
        self.client_frame = self.frame_size if client_rate is None else stream_pair_geometry(client_rate, CODEC_RATE, self.frame_size)
        self._rs_in = self._rs_out = None
        self.n_user = lm_gen.lm_model.num_codebooks - lm_gen.lm_model.dep_q - 1
        self._dec = None
        from . import ops
        self.fuse = bool(ops.PIPELINE_FUSE)     # one graph per frame once the delay line is full (False: the three module calls, as the reference loops)
        self._fused, self._gate = None, None
        self.last_codes: Optional[torch.Tensor] = None      # what the encoder emitted for the last frame, [B, K, 1] (valid until the next step)
        self.last_tokens: Optional[torch.Tensor] = None     # the LM's delay-aligned tokens of the last frame, [B, 1 + dep_q] (None inside the delay)
        # the packed route (step_packed): one record per row in, one out, REC bytes apart; its buffers belong to the session
        self.record_stride = record_stride(self.client_frame)
        self._mode: Optional[str] = None                 # "step" or "packed": a session takes its frames one way
        self._fmt = self._staged_dev = self._records_dev = self._records_host = self._pcm_in = self._no_tokens = self._done = None

    def __enter__(self):
        # encode touches only the encoder-side modules' states and decode only the decoder-side ones: one context serves both
        self._mimi_ctx = self.mimi.streaming(self.batch_size, per_stream=True) if self.per_stream else self.mimi.streaming(self.batch_size)
        self._mimi_ctx.__enter__()
        self._lm_ctx = self.lm_gen.streaming(self.batch_size, per_stream=True) if self.per_stream else self.lm_gen.streaming(self.batch_size)
        try:
            self._lm_ctx.__enter__()
        except Exception:
            self._mimi_ctx.__exit__(None, None, None)
            raise
        self._frames, self._awaiting, self.stream_valid = [0] * self.batch_size, [], []
        self._fused, self.last_codes, self.last_tokens = None, None, None     # a graph of an earlier session points at that session's states
        self._mode = None
        self._fmt = self._staged_dev = self._records_dev = self._records_host = self._pcm_in = self._no_tokens = self._done = None
        self._gate = RecaptureGate(self.lm_gen.lm_model.device, every_frame=True)
        if self.client_rate is not None:
            dev = self.lm_gen.lm_model.device
            self._rs_in = StreamResampler(self.client_rate, CODEC_RATE, self.frame_size, self.batch_size, dev)
            self._rs_out = StreamResampler(CODEC_RATE, self.client_rate, self.client_frame, self.batch_size, dev)
        return self

    def __exit__(self, *exc):
        self._fused, self.last_codes, self.last_tokens = None, None, None        # (the captured frame keeps the session's state tensors alive)
        self._fmt = self._staged_dev = self._records_dev = self._records_host = self._pcm_in = self._no_tokens = self._done = None
        self._rs_in = self._rs_out = None
        self._lm_ctx.__exit__(*exc)
        self._mimi_ctx.__exit__(*exc)
        return False

    def _frame_fn(self, pcm: torch.Tensor) -> torch.Tensor:
        """The three stages of a frame back to back on the device (the function the fused graph captures): no host-side slicing,
        cloning or re-staging of the codes / tokens between them.  (A quantised LM -- ``LMModel.quantize_weights_`` -- runs its fp8 routes
        here as in ``LMGen.step``, the GEMV at one or two streams and the weight-only fp8 skinny GEMM above; an MXFP4 model reads its
        per-layer matrices as bf16 above two streams unless it opted in to the batched route (``mxfp4_batched``: the weight-only MXFP4
        skinny GEMM): the route is chosen inside ``_frame`` from the model's ``weight_dtype`` and that flag.)"""
        return self._frame_body(pcm)[0]

    def _frame_body(self, pcm: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (decoded PCM ``[B, 1, frame_size]``, the LM's delay-aligned tokens ``[B, 1 + dep_q]``)."""
        B = self.batch_size
        codes = self.mimi.quantizer.encode_nlc(self.mimi.encode_latent(pcm))          # [B, K, 1]
        self.last_codes = codes         # (inside the graph: a static buffer every replay refills)
        out, _ = self.lm_gen._frame(codes[:, :self.n_user, 0].contiguous())            # [B, 1 + dep_q]
        self.last_tokens = out
        audio = out[:, 1:]
        if self.per_stream:
            audio = self._decodable(audio)
        return self.mimi._decode(audio.reshape(B, -1, 1)), out

    def _decodable(self, audio_tokens: torch.Tensor) -> torch.Tensor:
        """The decoder runs for every row of a per-stream batch on every frame; a row inside its delay still holds the ring's
        ``ungenerated`` / initial ids (-2, ``card``), which are no codebook entries: clamp them into the codebook (identity on generated
        tokens).  What such a row decodes to is never returned (``step`` zero-fills it) and is wiped from its state before its first valid frame."""
        return audio_tokens.clamp(0, self.lm_gen.lm_model.card - 1)

    def reset_streams(self, rows) -> None:
        """Rows ``rows`` of a live per-stream session start a new conversation with the next frame: encoder side, LM and decoder side of
        those rows become those of a new session, the other rows do not notice.  All of it is eager in-place writes between two frames;
        state tensors keep their addresses, so the captured frame graph goes on replaying.  The rows' PCM is zero for their first
        ``max_delay`` frames (``stream_valid`` lists who is past it); from then on it equals a new session's fed the same frames."""
        if not self.per_stream:
            raise ValueError("reset_streams needs StreamingPipeline(..., per_stream=True)")
        if self.lm_gen._streaming_state is None:
            raise RuntimeError("reset_streams outside the session: enter the pipeline first")
        rows = check_rows(rows, self.batch_size)
        if not rows:
            return
        self.mimi.reset_streams(rows, side="both")
        self.lm_gen.reset_streams(rows)
        if self._rs_in is not None:
            self._rs_in.reset_rows(rows)
            self._rs_out.reset_rows(rows)
        for b in rows:
            self._frames[b] = 0
        self._awaiting = sorted(set(self._awaiting) | set(rows)) if self.lm_gen.max_delay > 0 else self._awaiting

    def set_stream_sampling(self, rows, **kw) -> None:
        """``LMGen.set_stream_sampling``: rows ``rows`` sample by these settings from the next frame on (an ``LMGen`` built with
        ``per_stream_sampling=True``; in-place table writes between two frames, the captured frame goes on replaying)."""
        self.lm_gen.set_stream_sampling(rows, **kw)

    def stream_sampling(self, b: int) -> dict:
        """``LMGen.stream_sampling``: row ``b``'s sampling settings."""
        return self.lm_gen.stream_sampling(b)

    def _reset_decoder_side(self, rows) -> None:
        self.mimi.reset_streams(rows, side="decoder")
        if self._rs_out is not None:
            self._rs_out.reset_rows(rows)

    def _finish(self, wav: Optional[torch.Tensor], valid: List[int]) -> Optional[torch.Tensor]:
        """Per-stream: the frame's PCM with the rows inside their delay zero-filled (``wav`` is already this call's own copy)."""
        self._frames = [n + 1 for n in self._frames]
        self.stream_valid = valid
        if wav is None:
            return None
        if len(valid) < self.batch_size:
            wav[[b for b in range(self.batch_size) if b not in valid]] = 0.0
        return wav

    def _frame_fn_rate(self, pcm: torch.Tensor) -> torch.Tensor:
        """``_frame_fn`` between the session's two rate conversions: client rate -> 24 kHz -> client rate, still one graph."""
        return self._rs_out.step(self._frame_fn(self._rs_in.step(pcm)))

    @torch.no_grad()
    def step(self, pcm: torch.Tensor) -> Optional[torch.Tensor]:
        """pcm fp32 ``[B, 1, 1920]`` -> generated pcm ``[B, 1, 1920]`` (or ``None`` during the first ``max_delay`` frames).

        Once the delay line is full and every module has run its two eager frames (streaming buffers allocated, in-place from then
        on) a frame is ONE captured graph -- encode, LM frame,
        decode -- fed by one copy of the PCM and read by one clone of the result; before that, and on CPU tensors, under
        ``NO_CUDA_GRAPH=1`` or with ``LMGen(check=True)``, the three module calls run as the reference's loop does (server.py:122-136).
        With a ``client_rate`` the frames are ``[B, 1, client_frame]`` at that rate in both directions."""
        if self._mode == "packed":
            raise ValueError("this session takes its frames through step_packed: step and step_packed may not be mixed in one session")
        self._mode = "step"
        rated = self.client_rate is not None        # (client_frame == frame_size without a client rate)
        assert pcm.shape == (self.batch_size, 1, self.client_frame), tuple(pcm.shape)
        gen = self.lm_gen
        state = gen._streaming_state
        valid: List[int] = []
        if self.per_stream:
            reset_now, valid, self._awaiting = restart_schedule(self._frames, self._awaiting, gen.max_delay)
            if reset_now:
                self._reset_decoder_side(reset_now)
        fused_ok = (self.fuse and pcm.is_cuda and state is not None and state.offset >= gen.max_delay + 2 and not gen.check
                    and self.mimi.code_layout == "bkt")
        if fused_ok:
            if self._gate.moved(state.offset) or self._fused is None:
                # the first capture follows the modules' own eager frames (the delay line: max_delay + 2 of them).  A RE-capture after the
                # device's persistent launches were retired takes launch-per-op paths that have not run in this session yet: one eager
                # frame first, so that their lazily created state and scratch exist before the capture
                self._fused = Graphed(self._frame_fn_rate if rated else self._frame_fn, warmup=0 if self._fused is None else 1)
            if not self._fused.disable:
                wav = self._fused(pcm.contiguous())
                state.offset += 1
                if self.per_stream:
                    state.frames = [n + 1 for n in state.frames]
                    return self._finish(wav.clone(), valid)
                return wav.clone()
        if rated:
            pcm = self._rs_in.step(pcm)
        codes = self.mimi.encode(pcm)                                   # [B, 8, 1]
        self.last_codes = codes
        tokens = self.lm_gen.step(codes[:, :self.n_user].contiguous())  # [B, 1 + dep_q, 1] or None
        self.last_tokens = None if tokens is None else tokens[:, :, 0]
        if self.per_stream:
            if tokens is None:
                return self._finish(None, valid)
            wav = self.mimi.decode(self._decodable(tokens[:, 1:]).contiguous())
            return self._finish(self._rs_out.step(wav).clone() if rated else wav, valid)
        if tokens is None:
            return None
        wav = self.mimi.decode(tokens[:, 1:].contiguous())
        return self._rs_out.step(wav).clone() if rated else wav         # (no output, and no outgoing conversion, during the delay)

    # ------------------------------------------------------------------------------------------------ the packed route (a served batch)

    def _packed_buffers(self) -> None:
        dev, B, REC = self.lm_gen.lm_model.device, self.batch_size, self.record_stride
        pin = dev.type == "cuda"
        self._fmt = torch.full((B,), -1, device=dev, dtype=torch.int32)
        self._staged_dev = torch.zeros(B, REC, device=dev, dtype=torch.uint8)
        self._records_dev = torch.zeros(B, REC, device=dev, dtype=torch.uint8)
        self._records_host = torch.zeros(B, REC, dtype=torch.uint8, pin_memory=pin)
        self._pcm_in = torch.zeros(B, 1, self.client_frame, device=dev, dtype=torch.float32)
        self._no_tokens = torch.zeros(B, self.lm_gen.lm_model.dep_q + 1, device=dev, dtype=torch.long)
        self._done = torch.cuda.Event() if pin else None

    def _packed_session(self) -> None:
        if not self.per_stream:
            raise ValueError("the packed route needs StreamingPipeline(..., per_stream=True): validity comes from the per-stream frame counters")
        if self.lm_gen._streaming_state is None:
            raise RuntimeError("the packed route outside the session: enter the pipeline first")
        if self._fmt is None:
            self._packed_buffers()

    def new_staged(self) -> torch.Tensor:
        """A zeroed pinned uint8 ``[B, REC]`` buffer for ``step_packed`` (the caller fills it: ``slots.pack_staged``)."""
        pin = self.lm_gen.lm_model.device.type == "cuda"
        return torch.zeros(self.batch_size, self.record_stride, dtype=torch.uint8, pin_memory=pin)

    def set_row_format(self, b: int, fmt: int) -> None:
        """The transport of row ``b`` of the packed route: -1 free row, 0 f32, 1 s16.  An eager write of one word of a device vector the
        captured frame reads: nothing is captured again."""
        self._packed_session()
        if not 0 <= int(b) < self.batch_size:
            raise ValueError(f"row {b} is outside the batch of {self.batch_size}")
        if int(fmt) not in (-1, 0, 1):
            raise ValueError(f"unknown row format {fmt!r}: -1 (free), 0 (f32) or 1 (s16)")
        self._fmt[int(b)] = int(fmt)

    def _frame_fn_packed(self) -> torch.Tensor:
        """The whole served frame on the device (what the packed route captures): records -> PCM, the frame, PCM + tokens -> records.  It
        takes no argument: it reads and writes the session's own static buffers, so a replay copies nothing."""
        from . import ops
        pcm = ops.frame_ingress(self._staged_dev, self._fmt, self._pcm_in)
        if self.client_rate is not None:
            pcm = self._rs_in.step(pcm)
        wav, out = self._frame_body(pcm)
        if self.client_rate is not None:
            wav = self._rs_out.step(wav)
        return ops.frame_egress(wav.contiguous(), out, self.lm_gen._streaming_state.offset_dev, self.lm_gen.max_delay, self._fmt,
                                self._records_dev)

    @torch.no_grad()
    def step_packed(self, staged_host: torch.Tensor) -> torch.Tensor:
        """One frame of a served batch: ``staged_host`` uint8 ``[B, REC]`` (pinned; one ingress record per row, ``rst_frame_ingress``) ->
        the pipeline's own pinned uint8 ``[B, REC]`` of egress records (``rst_frame_egress``), valid until the next call.  One non-blocking
        upload, the frame -- ONE graph under the conditions of ``step``, eager module calls before that --, one non-blocking download, one
        event wait.  The host side of a restart (``restart_schedule``, the second decoder-side reset) and ``stream_valid`` are ``step``'s."""
        from . import ops
        self._packed_session()
        if self._mode == "step":
            raise ValueError("this session takes its frames through step: step and step_packed may not be mixed in one session")
        self._mode = "packed"
        B, REC = self.batch_size, self.record_stride
        if staged_host.dtype != torch.uint8 or tuple(staged_host.shape) != (B, REC) or staged_host.is_cuda or not staged_host.is_contiguous():
            raise ValueError(f"step_packed takes a host uint8 [{B}, {REC}] buffer (new_staged()), got {staged_host.dtype} {tuple(staged_host.shape)} "
                             f"on {staged_host.device}")
        gen = self.lm_gen
        state = gen._streaming_state
        rated = self.client_rate is not None
        reset_now, valid, self._awaiting = restart_schedule(self._frames, self._awaiting, gen.max_delay)
        if reset_now:
            self._reset_decoder_side(reset_now)
        on_gpu = self._staged_dev.is_cuda
        self._staged_dev.copy_(staged_host, non_blocking=True)
        fused_ok = (self.fuse and on_gpu and state.offset >= gen.max_delay + 2 and not gen.check and self.mimi.code_layout == "bkt")
        done = False
        if fused_ok:
            if self._gate.moved(state.offset) or self._fused is None:
                self._fused = Graphed(self._frame_fn_packed, warmup=0 if self._fused is None else 1)      # (as in step)
            if not self._fused.disable:
                with torch.cuda.device(self._staged_dev.device):
                    self._fused()
                state.offset += 1
                state.frames = [n + 1 for n in state.frames]
                done = True
        if not done:
            pcm = ops.frame_ingress(self._staged_dev, self._fmt, self._pcm_in)
            if rated:
                pcm = self._rs_in.step(pcm)
            codes = self.mimi.encode(pcm)
            self.last_codes = codes
            tokens = gen.step(codes[:, :self.n_user].contiguous())
            self.last_tokens = None if tokens is None else tokens[:, :, 0]
            if tokens is None:
                # nobody is past the delay: every counter is <= max_delay, so the egress marks every record invalid and writes zeros
                ops.frame_egress(self._pcm_in, self._no_tokens, state.offset_dev, gen.max_delay, self._fmt, self._records_dev)
            else:
                wav = self.mimi.decode(self._decodable(tokens[:, 1:]).contiguous())
                if rated:
                    wav = self._rs_out.step(wav)
                ops.frame_egress(wav.contiguous(), tokens.reshape(B, -1), state.offset_dev, gen.max_delay, self._fmt, self._records_dev)
        self._finish(None, valid)
        self._records_host.copy_(self._records_dev, non_blocking=True)
        if self._done is not None:
            self._done.record()
            self._done.synchronize()
        return self._records_host
