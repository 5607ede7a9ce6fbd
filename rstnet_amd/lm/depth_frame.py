"""The depth phase of a frame for a depth transformer with per-step weights -- ``LMModel.depformer`` (models/model.py:188-225) or
``GPT.codecformer`` (models/llama_streaming.py:560-590): ``DepthDecoder`` runs it (both front ends delegate to the one their model
owns), ``DepthFrameTables`` are the pointer tables of ``rst_depth_decode_frame`` (the phase as one persistent launch,
csrc/lm_depth.hip): host arrays of device pointers, built once per weight version."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from .. import ops
from ..packed import _PackedCache


class DepthFrameTables:
    def __init__(self, dep, heads: Sequence[torch.Tensor], head_bias: Sequence[Optional[torch.Tensor]], emb: Sequence[torch.Tensor]):
        """``dep``: the ``StreamingTransformer`` (weights_per_step = dep_q); ``heads[k]`` bf16 ``[card, E]``; ``head_bias[k]`` fp32 ``[card]``
        or None; ``emb[k]`` bf16 ``[rows, E]`` = the embedding table of step k's INPUT token."""
        L, Q, E = len(dep.layers), dep.weights_per_step, dep.d_model
        assert len(heads) == Q and len(emb) == Q and len(head_bias) == Q
        self.L, self.dep_q, self.E, self.H = L, Q, E, dep.num_heads
        self.Hd = dep.layers[0].gating[0].linear_out.weight.shape[1]
        self.card = heads[0].shape[0]
        keep: List[torch.Tensor] = []

        def ptrs(ts):
            arr = (C.c_void_p * len(ts))()
            for i, t in enumerate(ts):
                if t is None:
                    arr[i] = None
                    continue
                assert t.is_cuda and t.is_contiguous(), "depth-frame tables need contiguous device tensors"
                keep.append(t)
                arr[i] = t.data_ptr()
            return arr
        for layer in dep.layers:
            att = layer.self_attn
            assert att.in_proj_weight.dtype == torch.bfloat16 and tuple(att.in_proj_weight.shape) == (Q * 3 * E, E)
            assert tuple(att.out_proj.weight.shape) == (Q * E, E)
            for g in layer.gating:
                assert tuple(g.linear_in.weight.shape) == (2 * self.Hd, E) and tuple(g.linear_out.weight.shape) == (E, self.Hd)
        self.in_proj = ptrs([l.self_attn.in_proj_weight for l in dep.layers])
        self.out_proj = ptrs([l.self_attn.out_proj.weight for l in dep.layers])
        self.norm1 = ptrs([l.norm1.alpha_f32() for l in dep.layers])
        self.norm2 = ptrs([l.norm2.alpha_f32() for l in dep.layers])
        self.gate_in = ptrs([l.gating[k].linear_in.weight for l in dep.layers for k in range(Q)])
        self.gate_out = ptrs([l.gating[k].linear_out.weight for l in dep.layers for k in range(Q)])
        for h, e in zip(heads, emb):
            assert h.dtype == torch.bfloat16 and tuple(h.shape) == (self.card, E) and e.dtype == torch.bfloat16 and e.shape[1] == E
        self.heads = ptrs(list(heads))
        self.head_bias = ptrs(list(head_bias)) if any(b is not None for b in head_bias) else None
        self.emb = ptrs(list(emb))
        self.emb_rows = (C.c_int * Q)(*[int(e.shape[0]) for e in emb])
        self.eps = float(dep.layers[0].norm1.eps)
        self.context = dep.context
        dev = heads[0].device
        # 4 words (csrc/persist.h): time-out codes of the frame in flight | frames repaired by the one-workgroup launch | OR of the
        # repaired frames' codes | reserved; registered with ops.persistent_poll
        self.status = ops.new_persistent_status(dev)
        self._keep = keep

    def repairs(self) -> int:
        """Frames whose hand-offs timed out and that the repair launch recomputed (reads the device words: synchronises)."""
        return int(self.status[1].item())

    def check(self) -> None:
        """Raises if any launch so far had a timed-out hand-off, repaired or not (reads the device status words: synchronises).  The
        tokens of a repaired frame are right; the check exists for tests and ``LMGen(check=True)`` runs that want to know."""
        st = self.status.tolist()
        if st[0] or st[1]:
            raise RuntimeError(f"rst_depth_decode_frame: hand-offs timed out ({st[1]} frame(s) repaired by the one-workgroup launch, codes "
                               f"{st[2]:#x}, in flight {st[0]:#x}); the device was shared with other work or the launch was not fully resident")


class DepthDecoder:
    """The depth phase of a frame, once for ``LMGen`` and ``GPTGen``: step ``k`` of ``dep_q`` = in-projection ``k`` of the temporal output +
    embedding of the previous token -> the per-step-weights transformer ``dep`` -> head ``k`` -> sampler.  Owned by the model; holds
    REFERENCES to its modules (``dep_q`` each; ``emb[0]`` is the text table, a head may carry a ``bias``), never copies of their weights."""

    def __init__(self, dep, in_proj: Sequence, emb: Sequence, heads: Sequence):
        assert len(in_proj) == len(emb) == len(heads) == dep.weights_per_step
        self.dep, self.in_proj, self.emb, self.heads = dep, in_proj, emb, heads
        self._in_cat, self._tables = _PackedCache(), _PackedCache()

    def _head_bias(self, k: int) -> Optional[torch.Tensor]:
        return self.heads[k].bias_f32() if getattr(self.heads[k], "bias", None) is not None else None

    def in_all(self) -> torch.Tensor:
        """``[dep_q * E, dim]``: the in-projections stacked (a second copy per weight version): ONE weight-streaming launch per frame."""
        ws = [m.weight for m in self.in_proj]
        return self._in_cat.get(tuple(ws), lambda: torch.cat([w.detach() for w in ws], 0).contiguous())

    def tables(self) -> DepthFrameTables:
        """Pointer tables of the persistent depth-frame launch, rebuilt when any weight they point at changes."""
        dep = self.dep
        params = [p for l in dep.layers for p in (l.self_attn.in_proj_weight, l.self_attn.out_proj.weight, l.norm1.alpha, l.norm2.alpha)]
        params += [g.linear_in.weight for l in dep.layers for g in l.gating] + [g.linear_out.weight for l in dep.layers for g in l.gating]
        params += [m.weight for m in self.heads] + [getattr(m, "bias", None) for m in self.heads] + [m.weight for m in self.emb]
        return self._tables.get(tuple(params), lambda: DepthFrameTables(
            dep, [m.weight for m in self.heads], [self._head_bias(k) for k in range(len(self.heads))], [m.weight for m in self.emb]))

    def check(self) -> None:      # ``DepthFrameTables.check`` of the tables built so far, if any
        if self._tables._val is not None:
            self._tables._val.check()

    def step_hidden(self, k: int, tokens: torch.Tensor, col: int, h: Optional[torch.Tensor], *, h_all: Optional[torch.Tensor] = None,
                    w8: Optional[tuple] = None, pos: Optional[torch.Tensor] = None, step_index: Optional[int] = None) -> torch.Tensor:
        """Depth step ``k`` up to its head: previous token ``tokens[:, col]`` (int64 ``[B, n]``), ``h`` fp32 ``[B, dim]`` -> ``[B, E]``.  ``h_all``
        (``h @ in_all().T``) replaces ``h``; ``w8``: fp8 copy of in-projection ``k``; ``pos`` / ``step_index``: as ``StreamingTransformer.step``."""
        E = self.dep.d_model
        add = h_all[:, k * E:(k + 1) * E] if h_all is not None else ops.lm_linear(h, self.in_proj[k].weight, w8=w8)
        return self.dep.step(None, step_index=step_index, pos=pos, embed=(add, self.emb[k].weight, tokens, col))

    def step_logits(self, k: int, tokens: torch.Tensor, col: int, h: Optional[torch.Tensor], **step) -> torch.Tensor:
        """``step_hidden`` + head ``k`` -> logits fp32 ``[B, card]``."""
        return ops.lm_linear(self.step_hidden(k, tokens, col, h, **step), self.heads[k].weight, bias=self._head_bias(k))

    def forward_local(self, start: torch.Tensor, sequence: torch.Tensor, transformer_out: torch.Tensor) -> torch.Tensor:
        """Teacher-forced depth logits: ``start`` = the text ids int64 ``[B, T]`` or their float embedding ``[B, T, E]``, ``sequence`` int64
        ``[B, dep_q, T]``, ``transformer_out`` ``[B, T, dim]`` -> ``[B, T, dep_q, card]``: ``dep_q`` steps over ``B * T`` rows on a throw-away
        ring that never fills."""
        B, K, T = sequence.shape
        assert K == len(self.heads), f"Sequence shape {sequence.shape} must match the moshi stream output."
        dep, N = self.dep, B * T
        saved = dep._streaming_state
        dep._streaming_state = dep._init_streaming_state(N, capacity=K + 1)
        try:
            h = transformer_out.reshape(N, -1).float().contiguous()
            outs = []
            for k in range(K):
                w = self.in_proj[k].weight
                if k == 0 and start.dtype != torch.long:
                    x = ops.lm_linear(h, w, res=start.reshape(N, -1).float().contiguous())
                else:
                    prev = start if k == 0 else sequence[:, k - 1]
                    x = ops.embed_sum(prev.reshape(N, 1).contiguous(), [self.emb[k].weight], [0], add=ops.lm_linear(h, w))
                outs.append(ops.lm_linear(dep.step(x), self.heads[k].weight, bias=self._head_bias(k)).view(B, T, 1, -1))
        finally:
            dep._streaming_state = saved
        return torch.cat(outs, dim=2)

    def decode_frame(self, tokens: torch.Tensor, h: torch.Tensor, noise: Optional[torch.Tensor], pos: torch.Tensor, *, use_sampling: bool,
                     temp: float, top_k: int, limits: Optional[torch.Tensor] = None, rings=None, w8: Optional[tuple] = None, keep=None,
                     persistent: bool = True, temps: Optional[torch.Tensor] = None, top_ks: Optional[torch.Tensor] = None) -> None:
        """The whole phase IN PLACE on ``tokens`` (int64 ``[B, >= dep_q + 1]``, any row stride): column 0 holds the text token, step k embeds
        column k and samples column k + 1.  ``h`` fp32 ``[B, dim]``; ``noise``: Exp(1) draws ``[B, dep_q * top_k]`` or None (greedy); ``pos``:
        int64 ``arange(dep_q)`` on the device (the steps are positions 0 .. dep_q - 1 of a ring that restarts every frame, as constant device
        scalars: no counter to zero and bump); ``limits`` int32 ``[dep_q]``: per-step id blanking, or ``[B, dep_q]``: per stream and step; ``w8``: the fp8 copy of ``in_all()``.
        ``rings``, the KV rings of the launch-per-op chain -- None: those installed on the transformer; a state: swapped in for the call; a
        callable ``B -> state``: called only if the chain runs.  ``keep``: the object whose ``tables`` attribute keeps the pointer tables
        alive (a captured frame embeds their device pointers).  ``persistent=False`` keeps the call off the one-launch route.  ``temps`` fp32
        ``[B]`` with ``top_ks`` int32 ``[B]``: one temperature (<= 0: greedy) and top-k per stream for every step's sampler (``ops.lm_sample_ps``;
        ``top_k`` is then the cap and the width of a step's noise block).  The persistent launch keeps scalar parameters, so such a call
        takes the launch-per-op chain at every batch size."""
        dep, Q = self.dep, len(self.heads)
        B, dev = tokens.shape[0], h.device
        h_all = ops.lm_linear(h, self.in_all(), w8=w8)      # the in-projections of all dep_q steps: one 8 x larger launch instead of eight
        Hd, card = dep.layers[0].gating[0].linear_out.weight.shape[1], self.heads[0].weight.shape[0]
        if (temps is None) != (top_ks is None):
            raise ValueError("decode_frame: per-stream sampling parameters come as a pair (temps, top_ks)")
        if ops.depth_frame_enabled(dev) and persistent and temps is None and \
                ops.depth_frame_supported(B, dep.d_model, dep.num_heads, Hd, card, Q, len(dep.layers), top_k, device=dev):
            # batch 1 / 2: the whole phase (dep_q x (L layers + head + sampler)) is ONE persistent launch whose ops hand their vectors
            # over in-kernel, on a dense [B, dep_q + 1] buffer; the slot -> position map follows the capacity of the rings in use
            dense = tokens if tokens.shape[1] == Q + 1 and tokens.is_contiguous() else tokens[:, :Q + 1].contiguous()
            st = dep._streaming_state if rings is None else rings
            tables = self.tables()
            if keep is not None:
                keep.tables = tables
            ops.depth_decode_frame(tables, h_all, dense, noise, use_sampling=use_sampling, temp=temp, top_k=top_k, eps=dep.layers[0].norm1.eps,
                                   context=dep.context, limits=limits, ring_cap=None if st is None or callable(st) else st.k[0].shape[2])
            if dense is not tokens:
                tokens[:, 1:Q + 1] = dense[:, 1:]
            return
        saved = dep._streaming_state
        if rings is not None:
            dep._streaming_state = rings(B) if callable(rings) else rings
        try:
            for k in range(Q):
                logits = self.step_logits(k, tokens, k, None, h_all=h_all, pos=pos[k:k + 1], step_index=k)
                nz = None if noise is None else noise[:, k * top_k:(k + 1) * top_k]
                limit_dev = None if limits is None else (limits[k:k + 1] if limits.dim() == 1 else limits[:, k])
                if temps is not None:
                    ops.lm_sample_ps(logits, top_k=top_k, noise=nz, temps=temps, top_ks=top_ks, out=tokens[:, k + 1], limit_dev=limit_dev)
                else:
                    ops.lm_sample(logits, use_sampling=use_sampling, temp=temp, top_k=top_k, out=tokens[:, k + 1], noise=nz, limit_dev=limit_dev)
        finally:
            dep._streaming_state = saved
