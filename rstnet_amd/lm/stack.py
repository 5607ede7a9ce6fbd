"""The ring transformer pass that ``StreamingTransformer`` (lm/model.py: Moshi-style temporal and depth transformers) and
``LLAMAStreamingTransformer`` (lm/gpt.py: the litgpt-style backbone) share: the KV-ring state and its one constructor, the window and
route rules of a multi-position call, and the one launch chain over the layers.  A front end describes its attention (``Geometry``)
and its layers (``LayerView``: weights, biases, stored copies, adapters); which kernels run follows from those and from the route."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import ops

KV_DTYPES = (torch.float32, torch.bfloat16)
ROUTE_DECODE = "decode"                  # T = 1: lm_attn_decode (rotation, append, attention and split reduction in one launch)
ROUTE_DECODE_FUSED = "decode_fused"      # T = 1 on a short un-rotated ring (ops.gemv_attn_supported): the attention is the out-projection's prologue
ROUTE_APPEND_FIRST = "append_first"      # lm_rope_append, then attention over the ring: fp32 rings that the chunk does not fill
ROUTE_PREFILL = "prefill"                # lm_attn_prefill against ring + chunk, then lm_ring_append (csrc/lm_prefill.hip)


@dataclass
class _StepState:
    k: List[torch.Tensor]      # per layer [B, G, cap, D] ring (fp32 or bf16)
    v: List[torch.Tensor]
    pos: torch.Tensor          # int64 [1] on device: steps appended so far (= position of the next step); per-stream state: int64 [B]
    scratch: Optional[tuple] = None   # (split workspace, arrival counters) of the long-ring attention kernel
    # host mirror of `pos`.  Graph replays move `pos` without running Python: whoever replays a captured step keeps the mirror in step
    # (LMGen through temporal_base, GPT / GPTGen through lm.stack.counted_step) -- GPT chooses the route of a T > 1 call from it
    offset_cpu: int = 0
    tables: object = None             # ops.TemporalFrameTables of the persistent batch-1 launch (built at the first step that takes it)
    tables_key: object = None
    per_stream: bool = False          # `pos` holds one position per stream: every T > 1 call attends before it appends, chunk by chunk

    def reset(self) -> None:
        self.pos.zero_()
        self.offset_cpu = 0

    @classmethod
    def make(cls, batch: int, kv_heads: int, heads: int, head_dim: int, cap: int, dtype: torch.dtype, device, layers: int,
             per_stream: bool = False) -> "_StepState":
        """Zeroed rings ``[batch, kv_heads, cap, head_dim]`` per layer; rings of more than 64 slots also get the split scratch of the
        long-ring decode kernel (one partial per query head and split).  ``per_stream``: ``pos`` is int64 ``[batch]``, one position per
        stream -- its multi-position calls all take ``ROUTE_PREFILL``, whose kernels serve head size 64 or 128 only."""
        if per_stream and head_dim not in (64, 128):
            raise ValueError(f"per-stream positions: head size {head_dim} is outside the multi-position attention kernels (64 or 128)")
        shape = (batch, kv_heads, cap, head_dim)
        scratch = None
        if cap > 64:
            splits = ops.lm_attn_splits(cap, batch * heads)
            scratch = (torch.empty(batch, heads, splits, head_dim + 2, device=device),
                       torch.zeros(batch, heads, device=device, dtype=torch.int32))
        return cls([torch.zeros(shape, device=device, dtype=dtype) for _ in range(layers)],
                   [torch.zeros(shape, device=device, dtype=dtype) for _ in range(layers)],
                   torch.zeros(batch if per_stream else 1, device=device, dtype=torch.long), scratch, per_stream=per_stream)


def check_kv_dtype(kv_dtype: torch.dtype, capacity: Optional[int] = None) -> None:
    """The one place that says which ring dtypes exist, and (given a capacity) which rings can hold them."""
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype {kv_dtype}: the KV rings are torch.float32 or torch.bfloat16")
    if kv_dtype == torch.bfloat16 and capacity is not None and capacity <= 64:
        raise ValueError(f"kv_dtype=torch.bfloat16 on a ring of {capacity} slots: rings of <= 64 slots are read by the short-ring decode "
                         "kernel, which reads fp32 only; use kv_dtype=torch.float32 or a context above 64")


def prefill_window(context: Optional[int], cap: int) -> int:
    """Keys a query sees on a ring of ``cap`` slots, itself included: the context, and never more than ``cap - 1`` because the step
    kernels (like ``RingKVCache.complete``) hide the oldest slot of a full ring -- exactly what single steps see.
    ``GPTGen``'s rings of ``context + 1`` slots give the plain context."""
    return min(context, cap - 1) if context else cap - 1


def prefill_route(cap: int, pos: int, T: int, kv_dtype: torch.dtype) -> str:
    """Route of ``T`` new positions behind ``pos`` appended ones on a ring of ``cap`` slots.  Appending first is only right while the
    ring is not full after the chunk, ``pos + T < cap``, and its kernels read fp32 rings only.  (``pos + T > cap`` rewrites slots the
    chunk's earlier queries still see; at ``pos + T == cap`` nothing is rewritten, but those kernels apply the slot -> position map of
    the ring as it is AFTER the chunk to every query, and on a ring that is exactly full that map hides the oldest slot, SURVEY Q1:
    position 0 is lost to queries that single steps let see it.)  Everything else attends before it appends."""
    if kv_dtype == torch.float32 and pos + T < cap:
        return ROUTE_APPEND_FIRST
    return ROUTE_PREFILL


def prefill_chunks(cap: int, pos: int, T: int, kv_dtype: torch.dtype, chunk: int) -> list:
    """``[(t0, Tc, route)]`` of a ``T``-position call: a call that appends first as a whole stays ONE pass (the launches it always
    took); otherwise position chunks of ``min(chunk, cap)``, each with its own route."""
    if prefill_route(cap, pos, T, kv_dtype) == ROUTE_APPEND_FIRST:
        return [(0, T, ROUTE_APPEND_FIRST)]
    step = min(chunk, cap)
    return [(t0, min(step, T - t0), prefill_route(cap, pos + t0, min(step, T - t0), kv_dtype)) for t0 in range(0, T, step)]


def per_stream_chunks(cap: int, T: int, chunk: int) -> list:
    """``[(t0, Tc, ROUTE_PREFILL)]`` of a ``T``-position call on a per-stream state: chunks of ``min(chunk, cap)``, every one attending
    before it appends -- right at any fill level, so no position has to be known on the host.  A one-position tail stays on this route
    too: the decode kernels know no lengths."""
    step = min(chunk, cap)
    return [(t0, min(step, T - t0), ROUTE_PREFILL) for t0 in range(0, T, step)]


def chunk_advance(lengths: Sequence[int], t0: int, Tc: int) -> list:
    """Positions each stream takes from the chunk ``[t0, t0 + Tc)`` of a call with per-stream ``lengths``: ``clamp(len - t0, 0, Tc)`` --
    the host statement of what ``lm_ring_append_ragged(lengths=, t0=)`` appends and ``run_layers`` adds to ``st.pos``."""
    return [max(0, min(Tc, int(n) - t0)) for n in lengths]


def counted_step(st: _StepState, step, *args):
    """Run ONE T = 1 step of the global transformer through ``step`` -- a ``Graphed`` callable or a plain one -- and leave the host
    mirror ``st.offset_cpu`` one further, whether Python ran (warm-up, capture, eager: ``run_layers`` counted already) or a graph was
    replayed (the device counter ``st.pos`` moved, no Python ran).  ``prefill_chunks`` decides the route of a later ``T > 1`` call from
    that mirror without a device synchronisation, and a mirror that lags sends a chunk across the wrap down the append-first route:
    wrong values, no error.  So EVERY caller that may replay a captured step goes through here, and code that moves ``st.pos`` by hand
    (a benchmark that seeds a full ring) sets ``st.offset_cpu`` with it.  A per-stream state (``st.per_stream``) never consults the
    mirror or ``prefill_chunks``: its streams stand at different positions, and its ``T > 1`` calls attend before they append
    (``per_stream_chunks``), which is right at any fill level."""
    at = st.offset_cpu
    out = step(*args)
    st.offset_cpu = at + 1
    return out


class Geometry(NamedTuple):
    """The attention of one transformer as its front end states it; nothing here is normalised on the way to the kernels."""
    heads: Optional[int]          # None: one key/value head per query head (rst_lm_attn_prefill_f32 / rst_lm_ring_append); H: the _gqa entry points, G == H included
    context: Optional[int]
    rope: bool
    max_period: float
    rope_dims: int = 0            # leading head dims that rotate (0 = all)
    litgpt_freqs: bool = False    # the prefill kernels rotate by ops.gpt_rope_freqs (the table litgpt evaluates), not by the Moshi table inside ops


class LoraBank(NamedTuple):
    """Unmerged adapters of one linear for several adapter sets at once, in kernel form (``GPT.load_adapter_bank``): row ``b`` of a call
    takes set ``ids[b]``, or none where the id is outside ``[0, n_sets)``.  ``ids`` is the model's ONE int32 device vector, shared by
    every view (``GPT.set_adapter_ids`` writes it in place, so captured graphs see new ids on their next replay)."""
    A_bank: torch.Tensor          # bf16 [n_sets, r', in]
    B_bank: torch.Tensor          # bf16 [n_sets, out, r']
    post_scale: float
    ids: torch.Tensor             # int32 [B]


class LinearView(NamedTuple):
    w: torch.Tensor
    bias: Optional[torch.Tensor] = None
    w8: Optional[tuple] = None        # stored fp8 / MXFP4 copy of ``w``: streamed by the batch <= 2 GEMV route; an fp8 pair and an ``ops.Mxfp4BatchedCopy`` also by the skinny GEMM above
    lora: Optional[tuple] = None      # unmerged adapter ``(A, B, post_scale)`` in kernel form, or a ``LoraBank``


class LayerView(NamedTuple):
    """One layer as the launch chain reads it: the fused in-projection (rows ``[Q | K | V]``), the out-projection, the stacked gate
    input, the MLP output, and the two norms as ``(alpha, eps)``."""
    qkv: LinearView
    out: LinearView
    fc: LinearView
    proj: LinearView
    norm1: Tuple[torch.Tensor, float]
    norm2: Tuple[torch.Tensor, float]


def _lora_add(y: torch.Tensor, x, ad, **prologue) -> torch.Tensor:
    """``y + B (scaling * (A P(x)))`` -- the unmerged LoRA branch (llama_streaming.py:136-143) as two thin products; with a ``LoraBank``
    every row takes its stream's adapter (rows ``b * T + t``: ``T`` rows per id), the update going into ``y`` in place."""
    if ad is None:
        return y
    if isinstance(ad, LoraBank):
        B = ad.ids.numel()
        if x.shape[0] % B:
            raise ValueError(f"adapter bank: {x.shape[0]} rows do not divide over the {B} streams of set_adapter_ids")
        T = x.shape[0] // B
        a = ops.lora_bank_shrink(x, ad.A_bank, ad.ids, rows_per_id=T, post_scale=ad.post_scale, **prologue)
        return ops.lora_bank_expand(a, ad.B_bank, ad.ids, y, rows_per_id=T)
    A, Bm, scale = ad
    a = ops.lm_linear(x, A, **prologue)
    if scale != 1.0:
        a = a * scale
    return ops.lm_linear(a, Bm, res=y)


def _linear(x: torch.Tensor, lin: LinearView, fp8: bool, res: Optional[torch.Tensor] = None, **prologue) -> torch.Tensor:
    return _lora_add(ops.lm_linear(x, lin.w, res=res, bias=lin.bias, fp8=fp8, w8=lin.w8, **prologue), x, lin.lora, **prologue)


def run_layers(x: Optional[torch.Tensor], T: int, st: _StepState, route: str, geo: Geometry, layers: Sequence[LayerView], *,
               pos: Optional[torch.Tensor] = None, embed: Optional[tuple] = None, fp8: bool = False,
               lengths: Optional[torch.Tensor] = None, t0: int = 0) -> torch.Tensor:
    """x fp32 ``[B*T, E]`` (row ``b*T + t``) -> ``[B*T, E]``: ``T`` consecutive positions per stream through every layer, on ``route``
    (``T == 1``: a decode route).  Per layer: in-projection with the RMSNorm prologue | attention and ring append of the route |
    out-projection | gated MLP -- the MLP as two plain products where it carries unmerged adapters, because the gate follows fc_1 / fc_2
    WITH their updates.  ``embed = (add, table, tokens, col)`` instead of ``x``: the input is ``add + table[tokens[:, col]]``, formed inside
    the first launch for batch <= 2.  ``fp8``: the linears run on the fp8 matrix-core path (``GPT.use_fp8``).  Advances ``st.pos`` /
    ``st.offset_cpu`` by ``T`` unless the caller owns the position (``pos``).  ``lengths`` (int32 ``[B]`` on the device, ``ROUTE_PREFILL`` on a
    per-stream state) with the offset ``t0`` of these ``T`` rows inside the call the lengths count from: stream ``b`` appends, and its
    position advances by, ``clamp(lengths[b] - t0, 0, T)`` rows; the outputs of its other rows are unspecified."""
    B = (x.shape[0] if x is not None else embed[0].shape[0]) // T
    cap, D = st.k[0].shape[2], st.k[0].shape[3]
    pos_t = st.pos if pos is None else pos
    if lengths is not None and (route != ROUTE_PREFILL or not st.per_stream or pos is not None):
        raise ValueError("run_layers: per-stream lengths need a per-stream state on the prefill route")
    rot = dict(rope=geo.rope, max_period=geo.max_period, rope_dims=geo.rope_dims)
    rope_table = window = freqs = None
    if route == ROUTE_DECODE and geo.rope and cap > 64:
        # the step's rotation once for all layers (long rings: the attention launches read it instead of evaluating 24 libm calls per lane)
        rope_table = ops.lm_rope_table(pos_t, D, max_period=geo.max_period, rope_dims=geo.rope_dims)
    if route == ROUTE_PREFILL:
        window = prefill_window(geo.context, cap)
        freqs = ops.gpt_rope_freqs(x.device, geo.max_period, geo.rope_dims) if geo.litgpt_freqs else None
    qkv = None
    if embed is not None:
        add, table, tokens, col = embed
        if B <= 2 and table.shape[1] <= 4096 and table.shape[1] % 8 == 0:
            qkv, x = ops.gemv_embed(add, table, tokens, col, layers[0].qkv.w, alpha=layers[0].norm1[0], eps=layers[0].norm1[1])
        else:
            x = ops.embed_sum(tokens, [table], [col], add=add)        # (a column block of h_all is read in place: no copy launch)
    for l, ly in enumerate(layers):
        if l > 0 or qkv is None:
            qkv = _linear(x, ly.qkv, fp8, prologue=ops.PROLOGUE_RMSNORM, alpha=ly.norm1[0], eps=ly.norm1[1])
        k, v = st.k[l], st.v[l]
        if route == ROUTE_DECODE_FUSED:
            x = ops.gemv_attn(qkv, k, v, pos_t, ly.out.w, context=geo.context, res=x)
        else:
            if route == ROUTE_DECODE:
                a = ops.lm_attn_decode(qkv, k, v, pos_t, context=geo.context, scratch=st.scratch, heads=geo.heads,
                                       packed=B > 2 and not fp8 and not isinstance(ly.out.lora, LoraBank),      # (the bank's shrink reads fp32 rows)
                                       rope_table=rope_table, **rot)
            elif route == ROUTE_PREFILL:
                q3 = qkv.view(B, T, -1)
                a = ops.lm_attn_prefill(q3, k, v, pos_t, window=window, heads=geo.heads, freqs=freqs, **rot)
                # after the attention, in stream order: the slot of position pos + t still held position pos + t - cap
                if lengths is None:
                    ops.lm_ring_append(q3, k, v, pos_t, heads=geo.heads, freqs=freqs, **rot)
                else:
                    ops.lm_ring_append_ragged(q3, k, v, pos_t, heads=geo.heads, freqs=freqs, lengths=lengths, t0=t0, **rot)
            else:
                q = ops.lm_rope_append(qkv.view(B, T, -1), k, v, pos_t, heads=geo.heads, **rot)
                a = ops.attention(q, k, v, pos_dev=pos_t, ring=True, context=geo.context).view(B * T, -1)
            x = _linear(a, ly.out, fp8, res=x)
        if ly.fc.lora is None and ly.proj.lora is None:
            x = ops.lm_gated_pair(x, ly.fc.w, ly.proj.w, alpha=ly.norm2[0], eps=ly.norm2[1], res=x, bias_in=ly.fc.bias, bias_out=ly.proj.bias,
                                  fp8=fp8, w8_in=ly.fc.w8, w8_out=ly.proj.w8)
        else:
            u = _linear(x, ly.fc, fp8, prologue=ops.PROLOGUE_RMSNORM, alpha=ly.norm2[0], eps=ly.norm2[1])
            x = _linear(u, ly.proj, fp8, res=x, prologue=ops.PROLOGUE_SILU_GATE)
    if pos is None:
        st.pos.add_(T if lengths is None else (lengths - t0).clamp_(0, T))
        st.offset_cpu += T
    return x


def run_chunks(x: torch.Tensor, B: int, st: _StepState, plan: Sequence[tuple], geo: Geometry, layers: Sequence[LayerView], fp8: bool = False,
               lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x fp32 ``[B*T, E]`` -> ``[B*T, E]``: one ``run_layers`` pass per ``(t0, Tc, route)`` of ``plan``, which covers the ``T`` positions in
    order; ``lengths``: per-stream lengths of the whole call (each pass gets them with its ``t0``)."""
    if len(plan) == 1:
        return run_layers(x, plan[0][1], st, plan[0][2], geo, layers, fp8=fp8, lengths=lengths)
    xv = x.view(B, -1, x.shape[1])
    y = torch.empty_like(xv)
    for t0, Tc, route in plan:
        y[:, t0:t0 + Tc] = run_layers(xv[:, t0:t0 + Tc].reshape(B * Tc, -1), Tc, st, route, geo, layers, fp8=fp8, lengths=lengths,
                                      t0=t0).view(B, Tc, -1)
    return y.view(x.shape)
