"""Streaming generation for the ``GPT`` backbone: the offline loop of ``MLLM_v2/infer_no_streaming.py:168-323``
(``InferenceImp.__call__`` + ``reverse_delay``) with the same prompt handling, sampling rules and stop rule, but O(T):

  * the prompt ``[initial frame | prefix]`` is pushed through the global transformer ONCE (prefill: all positions per launch,
    bf16-MFMA skinny GEMMs + multi-query ring attention), every generated frame afterwards is one graph-replayed T = 1 step
    -- the reference re-runs ``forward_global`` over the whole sequence for every frame (:240);
  * the eight audio tokens of a frame come from eight depth-transformer steps (one captured graph, sampling included) -- the
    reference re-runs the teacher-forced ``forward_local`` over the whole prefix for every codebook (:259).

Both replacements are exact restatements of what the reference computes for the LAST position: its non-streaming passes see
positions 0..t with the causal + context mask and no ring, which a ring of capacity context + 1 (global) / dep_q + 1 (depth)
reproduces -- a ring that size never lets the `delta <= 0` slot-map quirk hide a key the mask would show.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import torch

from .. import ops
from ..graphs import Graphed as _Graphed, RecaptureGate
from .gpt import GPT, _GPTState, counted_step


def reverse_delay(x: torch.Tensor) -> torch.Tensor:
    """infer_no_streaming.py:311-323: codebooks 1..7 are generated one frame late; x ``[8, L]`` (or ``[L, 8]``) -> ``[8, L-1]``."""
    if x.shape[0] != 8:
        x = x.transpose(0, 1)
    out = torch.ones_like(x)
    out[0, :-1] = x[0, :-1]
    out[1:, :-1] = x[1:, 1:]
    return out[:, :-1]


@dataclass
class GenIds:
    """The literal ids of InferenceImp.__init__ (:178-183) and the sampling helpers; parameters here so that small test
    vocabularies can be used."""
    text_pad_token: int = 128003
    text_empty_token: int = 128002
    semantic_pad_token: int = 2049
    acoustic_pad_token: int = 2049
    n_audio_codes: int = 2048
    text_initial_token_id: Optional[int] = None      # None = model.text_initial_token_id (151655)


class GPTGen:
    """Frame-by-frame generator over a ``GPT`` for B concurrent streams (the counterpart of ``LMGen`` for the litgpt-style
    backbone): ``prefill`` pushes a prompt through the global transformer, ``frame`` draws the text token and the dep_q audio
    tokens of the next frame (one captured graph), ``advance`` feeds the completed frame back (one captured graph).
    Rings: capacity context + 1 (global) and dep_q + 1 (depth) -- see the module docstring."""

    def __init__(self, model: GPT, use_sampling: bool = True, temp: float = 0.8, temp_text: float = 0.7, top_k: int = 250,
                 top_k_text: int = 25, n_audio_codes: int = 2048,
                 noise: Optional[Callable[[str, int, int], torch.Tensor]] = None):
        self.model = model
        self.use_sampling, self.temp, self.temp_text, self.top_k, self.top_k_text = use_sampling, temp, temp_text, top_k, top_k_text
        self.n_audio_codes = n_audio_codes
        self.noise = noise           # test hook: Exp(1) draws (kind, g_idx, l_idx) -> [B, k]; disables graph capture
        self._saved = None
        self.tables = None           # the DepthFrameTables a captured frame points at (kept alive with the graph)
        self._limits: Optional[torch.Tensor] = None
        self._depth: Optional[_Graphed] = None
        self._fused: Optional[_Graphed] = None       # `step`: the whole frame as one graph on the session's token column `_col`
        self._col: Optional[torch.Tensor] = None
        self._regime = None
        self.B = 0

    def begin(self, batch_size: int, kv_dtype: Optional[torch.dtype] = None, adapter_ids=None, per_stream: bool = False) -> None:
        """Open a session of ``batch_size`` streams.  ``kv_dtype``: precision of the global KV rings (None = the model's ``kv_dtype``).
        ``adapter_ids``: the adapter set of every stream (``GPT.set_adapter_ids``; needs ``GPT.load_adapter_bank``) -- they may change
        during the session through ``set_adapter_ids``, the captured graphs read them from the device.  ``per_stream``: every stream keeps
        its own ring position (int64 ``[B]`` on the device) and its own row of id limits, so ``prefill(tokens, lengths)`` takes prompts of
        different lengths and ``reset_streams`` restarts single rows; head size 64 or 128 (refused here otherwise).  ``frame``, ``advance``,
        ``start`` and ``step`` are the same calls on either kind of session."""
        m = self.model
        cfg, dev = m.config, m.device
        eager = self.noise is not None or dev.type != "cuda"
        # (refuses an unserved kv_dtype, or per-stream positions on an unserved head size, before anything changes)
        ring = m.transformer._make_state(batch_size, cfg.context + 1, kv_dtype, per_stream=per_stream)
        if adapter_ids is not None:
            m.set_adapter_ids(adapter_ids)
        m._bank_rows(batch_size)      # (a loaded bank: one id per stream, in place before a step is captured)
        self._saved = (m.transformer._streaming_state, m._streaming_state, m.codecformer._streaming_state)
        m.transformer._streaming_state = ring
        m._streaming_state = _GPTState(_Graphed(m._global_step, disable=eager))
        m.codecformer._streaming_state = m.codecformer._init_streaming_state(batch_size, capacity=cfg.dep_q + 1)
        self._limits = torch.full((batch_size, cfg.dep_q) if per_stream else (cfg.dep_q,), self.n_audio_codes + 1, device=dev, dtype=torch.int32)
        self._depth_pos = torch.arange(cfg.dep_q, device=dev, dtype=torch.long)
        self._depth = _Graphed(self._depth_frame, disable=eager)
        self._regime, self.B, self._eager = None, batch_size, eager
        self._frames, self._gate = 0, RecaptureGate(dev)      # (`frame` and `step` share the frame counter and the gate)

    def end(self) -> None:
        m = self.model
        m.transformer._streaming_state, m._streaming_state, m.codecformer._streaming_state = self._saved
        self._saved = None
        self._fused = self._col = None       # the fused frame graph of `start` / `step` belongs to the session that ends here

    def _exp_noise(self, kind: str, g_idx: int, l_idx: int, B: int, k: int) -> Optional[torch.Tensor]:
        if not self.use_sampling:
            return None
        if self.noise is not None:
            return self.noise(kind, g_idx, l_idx).reshape(B, k).to(self.model.device, torch.float32).contiguous()
        return torch.empty(B, k, device=self.model.device, dtype=torch.float32).exponential_(1)    # utils/sampling.py:44-46

    def _frame_noise(self, g_idx: int, B: int, with_text: bool) -> Optional[torch.Tensor]:
        """Exp(1) noise of one frame's samplers, ``[B, (k_text +) dep_q * k]``: ONE draw (utils/sampling.py:44-46 draws per call; the
        values are i.i.d. either way), or the test hook's per-sampler draws side by side."""
        if not self.use_sampling:
            return None
        cfg = self.model.config
        k_text, k_eff = min(self.top_k_text, cfg.padded_vocab_size), min(self.top_k, cfg.audio_card)
        if self.noise is not None:
            parts = [self._exp_noise("text", g_idx, 0, B, k_text)] if with_text else []
            return torch.cat(parts + [self._exp_noise("audio", g_idx, l_idx, B, k_eff) for l_idx in range(cfg.dep_q)], 1)
        n = (k_text if with_text else 0) + cfg.dep_q * k_eff
        return torch.empty(B, n, device=self.model.device, dtype=torch.float32).exponential_(1)

    def _depth_into(self, tokens: torch.Tensor, h: torch.Tensor, noise: Optional[torch.Tensor]) -> None:
        """dep_q depth-transformer steps + sampling IN PLACE: ``tokens`` int64 ``[B, >= dep_q + 1]`` (any row stride) holds the text
        token in column 0; step l embeds column l and samples column l + 1 (the layout of ``LMGen._depth``).  ``noise``: Exp(1)
        draws ``[B, dep_q * k]`` or None (greedy)."""
        m = self.model
        # on the rings `begin` installed on the codecformer (capacity dep_q + 1, see the module docstring); this generator keeps the tables
        m.depth_decoder.decode_frame(tokens, h, noise, self._depth_pos, use_sampling=self.use_sampling, temp=self.temp,
                                     top_k=min(self.top_k, m.config.audio_card), limits=self._limits, keep=self)

    def _depth_frame(self, text_token: torch.Tensor, h: torch.Tensor, g_idx: int = 0) -> torch.Tensor:
        """dep_q depth-transformer steps + sampling: text_token int64 [B], h fp32 [B, n_embd] -> tokens int64 [B, dep_q]."""
        (B,) = text_token.shape
        tokens = torch.empty(B, self.model.config.dep_q + 1, device=text_token.device, dtype=torch.long)
        tokens[:, 0] = text_token
        self._depth_into(tokens, h, self._frame_noise(g_idx, B, with_text=False))
        return tokens[:, 1:].contiguous()

    # ---- the whole frame as ONE captured graph (serving / benchmark loop): global step of the previous frame's tokens, text sample,
    # dep_q depth steps with their samples -- fed by nothing, reading and writing the session's token column on the device
    def start(self, h: torch.Tensor, logits: torch.Tensor, g_idx: int = 0):
        """First frame after ``prefill``: samples it (``frame``) and loads it into the session's token column, from which ``step``
        continues.  Returns (text [B], audio [B, dep_q])."""
        text, audio = self.frame(h.contiguous(), logits.contiguous(), g_idx)
        cfg = self.model.config
        self._col = torch.full((h.shape[0], cfg.n_q + 1), self.model.initial_token_id, device=h.device, dtype=torch.long)
        self._col[:, 0] = text
        self._col[:, 1:cfg.dep_q + 1] = audio
        self._fused = _Graphed(self._step_fn, disable=self._eager)
        self._g_idx = g_idx
        return text, audio

    def _step_fn(self):
        m, cfg, col = self.model, self.model.config, self._col
        B = col.shape[0]
        # the completed frame through the global transformer (rows beyond dep_q carry the initial-token pad, infer_no_streaming.py:243-244);
        # its embedding launch reads the column before the samplers below overwrite it (stream order)
        h, logits = m._global_step(col)
        k_text = min(self.top_k_text, cfg.padded_vocab_size)
        noise = self._frame_noise(self._g_idx, B, with_text=True)
        ops.lm_sample(logits, use_sampling=self.use_sampling, temp=self.temp_text, top_k=k_text,
                      noise=None if noise is None else noise[:, :k_text], out=col[:, 0])
        self._depth_into(col, h, None if noise is None else noise[:, k_text:])
        return h, logits

    def step(self):
        """``advance`` of the previous frame + ``frame`` of the next one as ONE graph replay with no host-side tensor traffic: returns
        (text [B], audio [B, dep_q]) as VIEWS of the session's token column (valid until the next ``step``; clone to keep)."""
        col, cfg = self._col, self.model.config
        if col.is_cuda and not self._eager and self._gate.moved(self._frames):
            self._fused = _Graphed(self._step_fn)
        self._frames += 1
        self._g_idx += 1
        # (a graph replay advances the device counter only; `prefill` decides its route from the host mirror: lm.stack.counted_step)
        self.last_h, self.last_logits = counted_step(self.model.transformer._streaming_state, self._fused)
        return col[:, 0], col[:, 1:cfg.dep_q + 1]

    def set_blanking(self, wide: list) -> None:
        """Per-codebook id limit of the next frames: n_audio_codes + 1 where ``wide`` (sample_token_audio) else n_audio_codes
        (sample_token_audio_2048).  ``wide``: ``[dep_q]`` flags for every stream, or a ``[B][dep_q]`` table with one row per stream
        (``_limits`` is then ``[B, dep_q]``; a session that held ``[dep_q]`` limits drops its captured frames, which point at the old vector)."""
        n, dep_q = self.n_audio_codes, self.model.config.dep_q
        table = len(wide) > 0 and isinstance(wide[0], (list, tuple))
        if table and (len(wide) != self.B or any(len(r) != dep_q for r in wide)):
            raise ValueError(f"set_blanking: a per-stream table is [{self.B}][{dep_q}]")
        if not table and len(wide) != dep_q:
            raise ValueError(f"set_blanking: {len(wide)} flags for {dep_q} codebooks")
        if table and self._limits.dim() == 1:
            self._limits = self._limits.repeat(self.B, 1)
            self._depth = _Graphed(self._depth_frame, disable=self._eager)
            if self._fused is not None:
                self._fused = _Graphed(self._step_fn, disable=self._eager)
        lim = torch.tensor([[n + 1 if w else n for w in r] for r in (wide if table else [wide])], dtype=torch.int32)
        self._limits.copy_(lim if table else (lim[0] if self._limits.dim() == 1 else lim.expand(self.B, dep_q)))

    def reset_streams(self, rows: Sequence[int]) -> None:
        """Restart the given rows of a per-stream session at position 0, ready for ``prefill`` of a new prompt into them (the other rows
        taking length 0).  No ring is zeroed: at position 0 the slot -> position map shows a stream none of its slots, and every slot is
        appended to before a later position can see it."""
        st = self.model.transformer._streaming_state
        if st is None or not st.per_stream:
            raise ValueError("reset_streams needs a per-stream session (begin(..., per_stream=True))")
        rows = [int(r) for r in rows]
        if any(r < 0 or r >= self.B for r in rows):
            raise ValueError(f"reset_streams: rows {rows} outside [0, {self.B})")
        st.pos.index_fill_(0, torch.tensor(rows, dtype=torch.long).to(st.pos.device), 0)

    def prefill(self, tokens: torch.Tensor, lengths=None):
        """tokens int64 [B, K, T] -> (h [B, n_embd], logits [B, V]) of the LAST position, from which ``frame`` / ``start`` continue.
        Valid at any point of a live session: the T positions are appended behind whatever the session holds (a second turn, a wrapped
        ring included); the captured step graphs stay valid, positions being device scalars.
        ``lengths`` (list or integer tensor ``[B]``, ``0 <= len <= T``; a per-stream session): stream ``b`` consumes its first ``lengths[b]``
        positions and gets ``h`` / ``logits`` of ITS last position ``lengths[b] - 1``; a stream of length 0 takes nothing and gets
        unspecified values."""
        h, logits = self.model.forward_global(tokens, lengths)
        if lengths is None:
            return h[:, -1].contiguous(), logits[:, -1].contiguous()
        last = (torch.as_tensor(lengths).to(h.device, torch.long) - 1).clamp_(min=0)
        rows = torch.arange(h.shape[0], device=h.device)
        return h[rows, last].contiguous(), logits[rows, last].contiguous()

    def frame(self, h: torch.Tensor, logits: torch.Tensor, g_idx: int = 0):
        """(h, logits) of the last position -> (text token [B], audio tokens [B, dep_q]) of the next frame."""
        B = h.shape[0]
        if h.is_cuda and not self._eager and self._gate.moved(self._frames):
            # a device that had to repair frames of the persistent depth launch (csrc/persist.h) moves to the launch-per-op chain
            self._depth = _Graphed(self._depth_frame)
        self._frames += 1
        k_text = min(self.top_k_text, self.model.config.padded_vocab_size)
        text = ops.lm_sample(logits, use_sampling=self.use_sampling, temp=self.temp_text, top_k=k_text,
                             noise=self._exp_noise("text", g_idx, 0, B, k_text))
        audio = self._depth_frame(text, h, g_idx) if self._eager else self._depth(text, h)
        return text, audio

    def advance(self, text: torch.Tensor, audio: torch.Tensor):
        """Feed the completed frame (rows beyond dep_q carry the initial-token pad, infer_no_streaming.py:243-244)."""
        m = self.model
        cfg = m.config
        col = torch.full((text.shape[0], cfg.n_q + 1, 1), m.initial_token_id, device=text.device, dtype=torch.long)
        col[:, 0, 0] = text
        col[:, 1:cfg.dep_q + 1, 0] = audio
        h, logits = m.forward_global(col)
        return h[:, 0], logits[:, 0]


def blanking_regime(pre_gen_len: int, minlen: int, g_idx: int) -> int:
    """Blanking regime of frame ``g_idx`` behind a prefix of ``pre_gen_len`` positions (infer_no_streaming.py:264-283): 0 = the first frame,
    2049 everywhere; later frames: codebook 0 -> 2048, the others 2049 once ``pre_gen_len + g_idx > minlen`` (regime 1), else 2048 (regime 2)."""
    return 0 if g_idx == 0 else (1 if pre_gen_len + g_idx > minlen else 2)


def regime_wide(regime: int, dep_q: int) -> list:
    """The ``wide`` flags ``GPTGen.set_blanking`` takes for a regime of ``blanking_regime``."""
    return [True] * dep_q if regime == 0 else [l > 0 and regime == 1 for l in range(dep_q)]


class InferenceImp:
    """Same constructor and call convention as infer_no_streaming.py:168-190 (``args`` is kept for signature parity and unused).
    ``__call__(seq [K, L], mask)`` returns what the reference returns for task 'TTS' (``reverse_delay`` of the generated
    frames, ``[8, n-1]``); ``generate`` returns every product of the loop for any task."""

    def __init__(self, args, model: GPT, mode: str, temp_text: float, top_k_text: int, temp: float, top_k: int, task_name: str,
                 use_sampling: bool = True, ids: Optional[GenIds] = None,
                 noise: Optional[Callable[[str, int, int], torch.Tensor]] = None):
        self.model, self.args, self.mode, self.task_name = model, args, mode, task_name
        self.n_samples = 1
        self.use_sampling, self.temp_text, self.top_k_text, self.temp, self.top_k = use_sampling, temp_text, top_k_text, temp, top_k
        self.ids = ids or GenIds()
        self.noise = noise           # test hook: Exp(1) draws (kind, g_idx, l_idx) -> [1, k]; disables graph capture

    # ---- prompt handling (:190-230)
    def split_prompt(self, seq: torch.Tensor):
        ids, task = self.ids, self.task_name
        if task in ("text_only", "word_level_audio_text_alignment", "ASR"):
            pad_len = int(seq[0, 0:1, :].eq(ids.text_pad_token).int().sum())
        elif task in ("audio_only", "TTS"):
            pad_len = int(seq[0, 1:2, :].eq(ids.semantic_pad_token).int().sum())
        else:
            raise NotImplementedError
        seq = seq[:, :, :seq.shape[2] - pad_len]
        if task in ("text_only", "audio_only"):
            n = seq.shape[-1] // 2
            return seq[:, :, :n], n, n
        if task == "TTS":
            n_prefix = seq.shape[2] - int(seq[0, 0, :].eq(ids.text_empty_token).int().sum())
            n = seq.shape[2] - n_prefix
            return seq[:, :, :n_prefix], n, n
        if task == "ASR":
            n_prefix = int(seq[0, 0, :].eq(ids.text_empty_token).int().sum())
            return seq[:, :, :n_prefix + 1], seq.shape[2] - n_prefix + 13, seq.shape[2] - n_prefix - 13
        raise NotImplementedError

    @torch.no_grad()
    def generate(self, seq: torch.Tensor, mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """seq int64 ``[K, L]`` -> {'frames': [n, dep_q], 'text': [n]} (+ 'codes' = reverse_delay(frames) for task 'TTS' with
        8 codebooks)."""
        m, ids = self.model, self.ids
        cfg, dev = m.config, m.device
        seq = seq.to(dev).unsqueeze(0)
        prefix, maxlen, minlen = self.split_prompt(seq)
        init = m._get_initial_token()
        if ids.text_initial_token_id is not None:
            init[:, 0] = ids.text_initial_token_id
        pre_gen_len = prefix.shape[2]
        n_codes = ids.n_audio_codes
        gen = self._make_gen()
        gen.begin(1)
        frames, texts = [], []
        try:
            h, logits = gen.prefill(torch.cat([init, prefix], dim=-1))      # positions 0 .. pre_gen_len
            regime = None
            for g_idx in range(maxlen):
                # blanking regime of this frame (:264-283): first frame -> 2049 everywhere; later l = 0 -> 2048,
                # l > 0 -> 2049 once g_len > minlen else 2048
                new_regime = blanking_regime(pre_gen_len, minlen, g_idx)
                if new_regime != regime:
                    gen.set_blanking(regime_wide(new_regime, cfg.dep_q))
                    regime = new_regime
                text, audio = gen.frame(h.contiguous(), logits.contiguous(), g_idx)
                audio_host = audio[0].tolist()
                if g_idx > minlen and any(t >= n_codes for t in audio_host[3:]):     # the stop rule of :286-288
                    break
                frames.append(audio[0].clone())
                texts.append(text[0].clone())
                if g_idx + 1 == maxlen:
                    break
                h, logits = gen.advance(text, audio)
        finally:
            gen.end()
        out = {"frames": torch.stack(frames) if frames else torch.zeros(0, cfg.dep_q, dtype=torch.long, device=dev),
               "text": torch.stack(texts) if texts else torch.zeros(0, dtype=torch.long, device=dev)}
        if self.task_name == "TTS" and frames and cfg.dep_q == 8:
            out["codes"] = reverse_delay(out["frames"])
        return out

    def _make_gen(self) -> GPTGen:
        return GPTGen(self.model, self.use_sampling, self.temp, self.temp_text, self.top_k, self.top_k_text, self.ids.n_audio_codes, self.noise)

    @torch.no_grad()
    def generate_batch(self, seqs: Sequence[torch.Tensor]) -> List[Dict[str, torch.Tensor]]:
        """``generate`` for several prompts at once: seqs = B tensors int64 ``[K, L_i]`` of any lengths -> one dict per prompt with the keys
        and values ``generate`` gives that prompt alone.  One ragged prefill of ``[initial frame | prefix_i]`` on a per-stream session (every
        stream at its own positions: no padding enters a ring), then lock-step frames with a common ``g_idx``; blanking regime, ``maxlen``
        and the stop rule are per stream, the latter two on the host from ONE ``[B, dep_q]`` read per frame.  A finished stream keeps
        stepping and its tokens are dropped; the loop ends when every stream is done.  The noise test hook returns ``[B, k]`` here.  More
        prompts than one batch holds are the caller's loop."""
        m, ids = self.model, self.ids
        cfg, dev = m.config, m.device
        B = len(seqs)
        if B < 1:
            return []
        init = m._get_initial_token()
        if ids.text_initial_token_id is not None:
            init[:, 0] = ids.text_initial_token_id
        splits = [self.split_prompt(s.to(dev).unsqueeze(0)) for s in seqs]
        prompts = [torch.cat([init, prefix], dim=-1) for prefix, _, _ in splits]       # positions 0 .. pre_gen_len_i
        pre = [prefix.shape[2] for prefix, _, _ in splits]
        maxlen, minlen = [s[1] for s in splits], [s[2] for s in splits]
        lens = [p.shape[2] for p in prompts]
        tokens = torch.zeros(B, init.shape[1], max(lens), device=dev, dtype=torch.long)
        for b, p in enumerate(prompts):
            tokens[b, :, :lens[b]] = p[0]
        n_codes = ids.n_audio_codes
        frames: List[list] = [[] for _ in range(B)]
        texts: List[list] = [[] for _ in range(B)]
        done = [n <= 0 for n in maxlen]
        gen = self._make_gen()
        gen.begin(B, per_stream=True)
        try:
            h, logits = gen.prefill(tokens, lens)
            regimes, g_idx = None, 0
            while not all(done):
                # a finished stream keeps the regime it ended in: only a live stream's change is worth a write to the device
                new = [regimes[b] if done[b] and regimes is not None else blanking_regime(pre[b], minlen[b], g_idx) for b in range(B)]
                if new != regimes:
                    gen.set_blanking([regime_wide(r, cfg.dep_q) for r in new])
                    regimes = new
                text, audio = gen.frame(h.contiguous(), logits.contiguous(), g_idx)
                audio_host = audio.tolist()
                for b in range(B):
                    if done[b]:
                        continue
                    if g_idx > minlen[b] and any(t >= n_codes for t in audio_host[b][3:]):     # the stop rule of :286-288
                        done[b] = True
                        continue
                    frames[b].append(audio[b].clone())
                    texts[b].append(text[b].clone())
                    done[b] = g_idx + 1 == maxlen[b]
                if all(done):
                    break
                h, logits = gen.advance(text, audio)
                g_idx += 1
        finally:
            gen.end()
        outs = []
        for b in range(B):
            out = {"frames": torch.stack(frames[b]) if frames[b] else torch.zeros(0, cfg.dep_q, dtype=torch.long, device=dev),
                   "text": torch.stack(texts[b]) if texts[b] else torch.zeros(0, dtype=torch.long, device=dev)}
            if self.task_name == "TTS" and frames[b] and cfg.dep_q == 8:
                out["codes"] = reverse_delay(out["frames"])
            outs.append(out)
        return outs

    @torch.no_grad()
    def __call__(self, seq: torch.Tensor, mask: Optional[torch.Tensor] = None):
        if self.mode == "teacher-force":
            raise NotImplementedError("teacher-forced loss evaluation (training-side metric) is outside the generation path")
        out = self.generate(seq, mask)
        if self.task_name == "TTS":
            return out.get("codes", out["frames"])
        return out["frames"]
