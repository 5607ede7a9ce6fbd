"""``LMModel`` / ``LMGen`` -- drop-in for the streaming generation half of ``MLLM_v2/models/model.py`` (Moshi-style
RQ-Transformer: a temporal transformer over 17 token streams + a per-codebook depth transformer).

Same constructor keywords, ``state_dict`` keys (``emb.{i}.weight``, ``transformer.layers.{l}.self_attn.in_proj_weight``,
``...gating.linear_in.weight``, ``depformer.layers.{l}.gating.{k}.linear_out.weight``, ``linears.{k}.weight`` ...),
``forward`` / ``forward_local`` / ``forward_text`` / ``forward_depformer`` signatures and ``LMGen.step`` semantics (delayed token ring
cache, ``None`` for the first ``max_delay`` steps); ``LMGen.prefill`` takes in frames that already exist.  Inference only: no autograd.

Execution: weights bf16 in HBM, activations fp32, one decode step (T = 1) per call through the kernels of
``csrc/lm_*.hip`` -- or T positions per call through ``StreamingTransformer.run`` (``csrc/lm_prefill.hip``); a whole ``LMGen`` frame (token-ring update, ``forward_text``, the depth steps with their samplers, ring
commit) is captured into ONE HIP graph after a warm-up -- the reference wraps ``forward_text`` and ``depformer_step`` in two
``CUDAGraphed`` wrappers (``MLLM_v2/utils/compile.py:189-277``) and does the ring arithmetic on the host in between -- and the
environment flag ``NO_CUDA_GRAPH`` disables that (``compile.py:168-174``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
from torch import nn

from .. import ops
from ..codec.streaming import StreamingContainer, StreamingModule, check_rows
from ..graphs import Graphed as _Graphed, RecaptureGate
from ..packed import _PackedCache
from .depth_frame import DepthDecoder
from .stack import ROUTE_DECODE, ROUTE_DECODE_FUSED, ROUTE_PREFILL, Geometry, LayerView, LinearView, _StepState, prefill_window, run_chunks, run_layers


# positions per launch chain of the multi-position pass (StreamingTransformer.run); a chunk is also never longer than the ring
PREFILL_CHUNK = 256


def _gating_hidden(dim: int, dim_feedforward: int) -> int:
    """modules/gating.py:40-45."""
    return (21 * dim) // 8 if dim_feedforward == 4 * dim else (2 * dim_feedforward) // 3


def _wq(mod: nn.Module, name: str, tag: str) -> Optional[tuple]:
    q = getattr(mod, name + "_q" + tag, None)
    if q is None:
        return None
    w = getattr(mod, name)
    if getattr(mod, "_w" + tag + "_of").get(name) != (w.data_ptr(), w._version):
        setattr(mod, name + "_q" + tag, None)
        setattr(mod, name + "_s" + tag, None)
        return None
    return q, getattr(mod, name + "_s" + tag)


def _w8(mod: nn.Module, name: str = "weight") -> Optional[tuple]:
    """The ``(q, scale)`` fp8 copy of parameter ``name`` of ``mod`` (``LMModel.quantize_weights_``), or None.  The copy is dropped when
    the bf16 parameter was replaced or written since: it then no longer holds the same values."""
    return _wq(mod, name, "8")


def _w4(mod: nn.Module, name: str = "weight", batched: bool = False) -> Optional[tuple]:
    """The MXFP4 copy (``ops.Mxfp4Copy``) of parameter ``name`` of ``mod`` (``LMModel.quantize_weights_("mxfp4")``), or None; dropped
    like the fp8 copy of ``_w8`` when the bf16 parameter was replaced or written since.  ``batched``: the model opted in to the batched
    route, so the copy is handed out as an ``ops.Mxfp4BatchedCopy`` (same fields; ``ops.lm_linear`` streams it above two rows too)."""
    c = _wq(mod, name, "4")
    return None if c is None else (ops.Mxfp4BatchedCopy if batched else ops.Mxfp4Copy)(*c)


def _wcopy(mod: nn.Module, name: str, weight_dtype: str, batched: bool = False) -> Optional[tuple]:
    """The stored copy of a quantised model's matrix that ``ops.lm_linear`` / ``ops.lm_gated_pair`` stream instead of the bf16 parameter:
    under ``"mxfp4"`` the MXFP4 copy where the matrix has one (batch <= 2 GEMV route; above two rows that matrix is read as bf16 unless
    ``batched`` -- the model's ``mxfp4_batched`` -- hands the copy out as an ``ops.Mxfp4BatchedCopy``, which the weight-only MXFP4 skinny
    GEMM ``ops.gemm_skinny_mxfp4w`` streams there and in prefill), else the fp8 copy (heads; K no multiple of 32); under ``"fp8"`` the
    fp8 copy, which serves the batch <= 2 GEMVs and, above two rows and in prefill, the weight-only fp8 skinny GEMM (``ops.gemm_skinny_fp8w``); None for bf16."""
    if weight_dtype == "bf16":
        return None
    return (_w4(mod, name, batched) if weight_dtype == "mxfp4" else None) or _w8(mod, name)


def _attach_copy(mod: nn.Module, name: str, tag: str, q: torch.Tensor, scale: torch.Tensor) -> None:
    """``(q, scale)`` become the non-persistent buffers ``<name>_q<tag>`` / ``<name>_s<tag>`` of ``mod``, valid for the parameter as it is now."""
    w = getattr(mod, name)
    if not hasattr(mod, "_w" + tag + "_of"):
        setattr(mod, "_w" + tag + "_of", {})
    for suffix, t in (("_q" + tag, q), ("_s" + tag, scale)):
        if hasattr(mod, name + suffix):
            setattr(mod, name + suffix, t)
        else:
            mod.register_buffer(name + suffix, t, persistent=False)
    getattr(mod, "_w" + tag + "_of")[name] = (w.data_ptr(), w._version)


def adopt_state_dict(model: nn.Module, sd: Dict[str, torch.Tensor]) -> None:
    """The tensors of ``sd`` become the parameters of ``model`` (built on the meta device) WITHOUT being copied."""
    params = dict(model.named_parameters())
    missing = [k for k in params if k not in sd]
    unexpected = [k for k in sd if k not in params]
    if missing or unexpected:
        raise RuntimeError(f"state_dict mismatch: missing={missing[:5]} unexpected={unexpected[:5]}")
    for name, tensor in sd.items():
        mod = model
        *path, leaf = name.split(".")
        for part in path:
            mod = getattr(mod, part) if not part.isdigit() else mod[int(part)]
        assert tuple(getattr(mod, leaf).shape) == tuple(tensor.shape), name
        setattr(mod, leaf, nn.Parameter(tensor, requires_grad=False))


class _Weight(nn.Module):
    """Holder of a ``weight`` parameter (nn.Linear / nn.Embedding key layout); the arithmetic lives in the kernels."""

    def __init__(self, *shape: int, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(*shape, device=device, dtype=dtype), requires_grad=False)
        nn.init.normal_(self.weight, std=0.02)


class ScaledEmbedding(_Weight):
    """models/model.py:67-91 -- lookup with id -1 -> zeros, executed by rst_embed_sum_bf16."""

    def __init__(self, num_embeddings: int, embedding_dim: int, zero_idx: int = -1, device=None, dtype=None, **_):
        super().__init__(num_embeddings, embedding_dim, device=device, dtype=dtype)
        self.zero_idx = zero_idx

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        """ids int64 ``[...]`` -> fp32 ``[..., D]`` (callers that look a table up directly, e.g. infer_no_streaming.py:258)."""
        flat = input.reshape(-1, 1).contiguous()
        return ops.embed_sum(flat, [self.weight], [0]).view(*input.shape, self.weight.shape[1])


class RMSNorm(nn.Module):
    """rms_norm_f32 (modules/transformer.py:49-65, eps 1e-8); key ``alpha`` [1,1,D]."""

    def __init__(self, dim: int, eps: float = 1e-8, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.alpha = nn.Parameter(torch.ones(1, 1, dim, device=device, dtype=dtype), requires_grad=False)
        self._f32 = _PackedCache()

    def alpha_f32(self) -> torch.Tensor:
        return self._f32.get((self.alpha,), lambda: self.alpha.detach().float().reshape(-1).contiguous())


class ActivationGating(nn.Module):
    """modules/gating.py:25-51 (SiLU): keys ``linear_in.weight`` [2*hidden, dim], ``linear_out.weight`` [dim, hidden]."""

    def __init__(self, dim: int, dim_feedforward: int, device=None, dtype=None):
        super().__init__()
        hidden = _gating_hidden(dim, dim_feedforward)
        self.linear_in = _Weight(2 * hidden, dim, device=device, dtype=dtype)
        self.linear_out = _Weight(dim, hidden, device=device, dtype=dtype)


class _Attention(nn.Module):
    def __init__(self, dim: int, mult: int, device=None, dtype=None):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(mult * 3 * dim, dim, device=device, dtype=dtype), requires_grad=False)
        nn.init.normal_(self.in_proj_weight, std=0.02)
        self.out_proj = _Weight(mult * dim, dim, device=device, dtype=dtype)


class _Layer(nn.Module):
    def __init__(self, dim: int, dim_feedforward: int, weights_per_step: int, device=None, dtype=None):
        super().__init__()
        fk = {"device": device, "dtype": dtype}
        self.self_attn = _Attention(dim, weights_per_step or 1, **fk)
        self.norm1 = RMSNorm(dim, **fk)
        self.norm2 = RMSNorm(dim, **fk)
        if weights_per_step:
            self.gating = nn.ModuleList([ActivationGating(dim, dim_feedforward, **fk) for _ in range(weights_per_step)])
        else:
            self.gating = ActivationGating(dim, dim_feedforward, **fk)


class StreamingTransformer(StreamingModule[_StepState]):
    """Decode-step executor with the parameter layout of modules/transformer.py:595-690 (norm rms_norm_f32, SiLU gating,
    causal, rope or no positional embedding, optional per-step weights)."""

    def __init__(self, d_model: int, num_heads: int, num_layers: int, dim_feedforward: int, context: Optional[int],
                 positional_embedding: str, max_period: float = 10000.0, weights_per_step: int = 0, device=None, dtype=None,
                 kv_dtype: torch.dtype = torch.float32):
        super().__init__()
        # precision of the KV rings: bf16 = what the reference caches (RingKVCache in the model's dtype); rings of <= 64 slots
        # (the depth transformer, tiny test models) always stay fp32 -- their bytes do not matter and their kernel is fp32
        assert kv_dtype in (torch.float32, torch.bfloat16)
        self.kv_dtype = kv_dtype
        assert d_model % num_heads == 0
        if positional_embedding not in ("rope", "none"):
            raise NotImplementedError(f"positional_embedding={positional_embedding!r}")
        self.d_model, self.num_heads, self.context = d_model, num_heads, context
        self.rope, self.max_period, self.weights_per_step = positional_embedding == "rope", max_period, weights_per_step
        self.weight_dtype = "bf16"        # "fp8" / "mxfp4": LMModel.quantize_weights_ left copies on the layers; the chain route streams them
        self.mxfp4_batched = False        # "mxfp4" only: the MXFP4 copies are streamed above two rows too (quantize_weights_(..., batched=True))
        self.layers = nn.ModuleList([_Layer(d_model, dim_feedforward, weights_per_step, device=device, dtype=dtype)
                                     for _ in range(num_layers)])

    def _apply_named_streaming(self, fn) -> None:
        """As the ROOT of a walk this module is always visited: the reference skips a propagate=False root but still visits
        its layers (modules/streaming.py:67-84, relied on by ``with lm.depformer.streaming(B)``), and the per-layer states of
        the reference live in this module's single state."""
        fn("", self)

    def _init_streaming_state(self, batch_size: int, capacity: Optional[int] = None) -> _StepState:
        if self.context is None and not self.weights_per_step:
            raise RuntimeError("Cannot create a streaming KVCache without a context to estimate capacity.")
        cap = capacity or (self.context if self.context is not None else self.weights_per_step)
        H = self.num_heads
        # (a per-stream session, `streaming(batch_size, per_stream=True)`: one position per stream on the temporal rings; the depth rings
        # restart every frame for all streams and keep their scalar positions)
        return _StepState.make(batch_size, H, H, self.d_model // H, cap, self.kv_dtype if cap > 64 else torch.float32,
                               self.layers[0].norm1.alpha.device, len(self.layers),
                               per_stream=self._streaming_per_stream and not self.weights_per_step and capacity is None)

    def _geometry(self) -> Geometry:
        return Geometry(None, self.context, self.rope, self.max_period)

    def _views(self, k_idx: int = 0) -> List[LayerView]:
        """The layers as ``stack.run_layers`` reads them: with per-step weights the matrices of step ``k_idx``; of a quantised model also the
        fp8 / MXFP4 copies (never the depth transformer: its weights are not covered)."""
        E, Q = self.d_model, self.weights_per_step
        wd, bt = "bf16" if Q else self.weight_dtype, self.mxfp4_batched

        def view(layer):
            att, gate = layer.self_attn, layer.gating[k_idx] if Q else layer.gating
            w_in, w_out = att.in_proj_weight, att.out_proj.weight
            if Q:
                w_in, w_out = w_in.view(Q, 3 * E, E)[k_idx], w_out.view(Q, E, E)[k_idx]
            return LayerView(LinearView(w_in, w8=_wcopy(att, "in_proj_weight", wd, bt)), LinearView(w_out, w8=_wcopy(att.out_proj, "weight", wd, bt)),
                             LinearView(gate.linear_in.weight, w8=_wcopy(gate.linear_in, "weight", wd, bt)),
                             LinearView(gate.linear_out.weight, w8=_wcopy(gate.linear_out, "weight", wd, bt)),
                             (layer.norm1.alpha_f32(), layer.norm1.eps), (layer.norm2.alpha_f32(), layer.norm2.eps))
        return [view(layer) for layer in self.layers]

    def step(self, x: Optional[torch.Tensor], step_index: Optional[int] = None, pos: Optional[torch.Tensor] = None,
             embed: Optional[tuple] = None) -> torch.Tensor:
        """x fp32 ``[B, d_model]`` -> ``[B, d_model]``: one new time step through every layer.  ``pos`` (int64 device scalar):
        position of this step supplied by a caller that owns the loop (LMGen's depth steps are always positions 0 .. dep_q - 1);
        the module's own counter is then left alone.  ``embed = (add, table, tokens, col)`` instead of ``x``: the input is
        ``add + table[tokens[:, col]]`` (``add`` fp32 ``[B, d_model]``, any row stride) and is formed inside the first launch.

        Launches per layer -- batch <= 2: 4 for a short un-rotated ring (qkv GEMV | out-proj GEMV with the attention as its
        prologue | ffn-in GEMV with the gate | ffn-out GEMV), 5 otherwise (attention on its own); batch > 2: 5."""
        st = self._streaming_state
        if st is None:
            raise RuntimeError("the decode-step transformer only runs in streaming mode")
        E, H = self.d_model, self.num_heads
        B = x.shape[0] if x is not None else embed[0].shape[0]
        cap = st.k[0].shape[2]
        fused_attn = ops.gemv_attn_supported(B, H, E // H, cap, self.rope)
        k_idx = 0
        if self.weights_per_step:
            k_idx = st.offset_cpu if step_index is None else step_index
        if st.per_stream and pos is None:
            # one position per stream: the decode launch that reads them, at every batch size (never the fused short-ring form, never
            # the persistent launch -- both know one position per call)
            return run_layers(x, 1, st, ROUTE_DECODE, self._geometry(), self._views(k_idx), embed=embed)
        if B == 1 and x is not None and not self.weights_per_step and cap > 64 and ops.temporal_frame_wanted(st.offset_cpu):
            y = self._persistent_step(st, x, st.pos if pos is None else pos, cap)
            if y is not None:
                if pos is None:
                    st.pos.add_(1)
                    st.offset_cpu += 1
                return y
        return run_layers(x, 1, st, ROUTE_DECODE_FUSED if fused_attn else ROUTE_DECODE, self._geometry(), self._views(k_idx), pos=pos, embed=embed)

    def window(self, cap: int) -> int:
        """Keys a query sees on a ring of ``cap`` slots, itself included (``stack.prefill_window`` of this transformer's context)."""
        return prefill_window(self.context, cap)

    def run(self, x: torch.Tensor, B: int, T: int) -> torch.Tensor:
        """x fp32 ``[B*T, d_model]`` (row ``b*T + t``) -> ``[B*T, d_model]``: ``T`` new positions per stream through every layer, equal to
        the same positions fed to ``step`` one at a time.  Per chunk of ``PREFILL_CHUNK`` positions and layer: in-projection with the
        RMSNorm prologue | prefill attention against the ring plus the chunk | ring append | out-projection | gated MLP; the linears
        stream their weights once per 64 rows.  Advances the position counters by ``T``.  ``T == 1`` is ``step``."""
        st = self._streaming_state
        if st is None:
            raise RuntimeError("the decode-step transformer only runs in streaming mode")
        if self.weights_per_step:
            raise NotImplementedError("run() serves the temporal transformer; per-step-weights (depth) transformers advance by `step`")
        if T == 1:
            return self.step(x)
        assert x.shape == (B * T, self.d_model), (tuple(x.shape), B, T, self.d_model)
        chunk = min(PREFILL_CHUNK, st.k[0].shape[2])      # (this pass always attends before it appends and plans without the host counter)
        plan = [(t0, min(chunk, T - t0), ROUTE_PREFILL) for t0 in range(0, T, chunk)]
        return run_chunks(x, B, st, plan, self._geometry(), self._views())

    def _persistent_step(self, st: _StepState, x: torch.Tensor, pos_t: torch.Tensor, cap: int) -> Optional[torch.Tensor]:
        """All layers of a batch-1 step as ONE persistent launch (csrc/lm_temporal.hip) when the library serves the shape and the
        device's persistent launches are healthy; None -> the launch-per-op chain below.  Never for a quantised model: the persistent
        launch reads the bf16 weights and would stream twice the bytes of the chain."""
        if self.weight_dtype != "bf16":
            return None
        E, H = self.d_model, self.num_heads
        Hd = self.layers[0].gating.linear_out.weight.shape[1]
        w0 = self.layers[0].self_attn.in_proj_weight
        if w0.dtype != torch.bfloat16 or not ops.temporal_frame_supported(1, E, H, Hd, len(self.layers), cap, st.k[0].dtype == torch.bfloat16, x.device):
            return None
        key = (ops.persistent_epoch(x.device),) + tuple((ly.self_attn.in_proj_weight.data_ptr(), ly.self_attn.in_proj_weight._version,
                                                          ly.gating.linear_in.weight.data_ptr()) for ly in self.layers)
        if st.tables is None or st.tables_key != key:
            st.tables = ops.TemporalFrameTables(
                [dict(in_proj=ly.self_attn.in_proj_weight, out_proj=ly.self_attn.out_proj.weight, gate_in=ly.gating.linear_in.weight,
                      gate_out=ly.gating.linear_out.weight, norm1=ly.norm1.alpha_f32(), norm2=ly.norm2.alpha_f32(), k_cache=st.k[l],
                      v_cache=st.v[l]) for l, ly in enumerate(self.layers)],
                H=H, context=self.context, eps=self.layers[0].norm1.eps)
            st.tables_key = key
        rope_table = ops.lm_rope_table(pos_t, E // H, max_period=self.max_period) if self.rope else None
        return ops.temporal_decode_frame(st.tables, x, pos_t, rope_table)


class ModelConfig:
    def __init__(self, model_type):
        self.model_type = model_type


class LMModel(StreamingContainer):
    """models/model.py:98-225 (constructor keywords identical; only the inference-relevant ones are interpreted)."""

    def __init__(self, delays: List[int] = [0], n_q: int = 8, dep_q: int = 8, card: int = 1024, text_card: int = 32000,
                 dim: int = 128, num_heads: int = 8, hidden_scale: float = 4, norm: str = "layer_norm", norm_emb: bool = False,
                 bias_proj: bool = False, depformer_dim: int = 256, depformer_dim_feedforward=None,
                 depformer_multi_linear: bool = False, depformer_weights_per_step: bool = False, depformer_pos_emb: str = "sin",
                 existing_text_padding_id: Optional[int] = None, context: Optional[int] = None, device=None,
                 dtype=torch.bfloat16, kv_dtype: torch.dtype = torch.bfloat16, **kwargs):
        super().__init__()
        self.kv_dtype = kv_dtype      # temporal KV rings: bf16 like the reference's cache (fp32 on request, e.g. fp32 parity runs)
        if norm != "rms_norm_f32" or norm_emb or bias_proj:
            raise NotImplementedError("the decode path implements norm='rms_norm_f32', norm_emb=False, bias_proj=False")
        if kwargs.get("gating", "silu") != "silu" or kwargs.get("depformer_gating", "silu") != "silu":
            raise NotImplementedError("SiLU gating only")
        if not (depformer_multi_linear and depformer_weights_per_step and depformer_pos_emb == "none"):
            raise NotImplementedError("depth transformer: multi_linear + weights_per_step + pos_emb 'none' (the Moshi / RSTnet setup)")
        if kwargs.get("layer_scale") is not None or kwargs.get("depformer_layer_scale") is not None:
            raise NotImplementedError("layer_scale")
        self.n_q, self.dep_q, self.card, self.text_card = n_q, dep_q, card, text_card
        assert len(delays) == self.num_codebooks, "unexpected number of delays"
        self.delays, self.dim, self.context = list(delays), dim, context
        self.existing_text_padding_id = existing_text_padding_id
        fk = {"device": device, "dtype": dtype}
        self.emb = nn.ModuleList([ScaledEmbedding(card + 1, dim, **fk) for _ in range(n_q)])
        self.text_emb = ScaledEmbedding(text_card + 1, dim, **fk)
        self.text_linear = _Weight(text_card + (1 if existing_text_padding_id is None else 0), dim, **fk)
        self.transformer = StreamingTransformer(dim, num_heads, kwargs["num_layers"], int(hidden_scale * dim), context,
                                                kwargs.get("positional_embedding", "sin"), kwargs.get("max_period", 10000.0),
                                                kv_dtype=kv_dtype, **fk)
        self.out_norm = RMSNorm(dim, **fk)
        self.depformer_multi_linear = depformer_multi_linear
        self.depformer_in = nn.ModuleList([_Weight(depformer_dim, dim, **fk) for _ in range(dep_q)])
        self.depformer_emb = nn.ModuleList([ScaledEmbedding(card + 1, depformer_dim, **fk) for _ in range(dep_q - 1)])
        self.depformer_text_emb = ScaledEmbedding(text_card + 1, depformer_dim, **fk)
        if depformer_dim_feedforward is None:
            depformer_dim_feedforward = int(hidden_scale * depformer_dim)
        self.depformer = StreamingTransformer(depformer_dim, kwargs.get("depformer_num_heads", num_heads),
                                              kwargs.get("depformer_num_layers", kwargs["num_layers"]), depformer_dim_feedforward,
                                              None, "none", kwargs.get("depformer_max_period", 10000.0), weights_per_step=dep_q, **fk)
        self.depformer.set_streaming_propagate(False)
        self.linears = nn.ModuleList([_Weight(card, depformer_dim, **fk) for _ in range(dep_q)])
        self.config = ModelConfig(model_type="lora")
        self._in_cat8 = _PackedCache()
        self.weight_dtype = "bf16"
        self.mxfp4_batched = False        # quantize_weights_("mxfp4", batched=True): the MXFP4 copies also serve the routes above two rows
        # the depth phase of a frame (lm.depth_frame.DepthDecoder; LMGen._depth and the methods below delegate to it)
        self.depth_decoder = DepthDecoder(self.depformer, self.depformer_in, [self.depformer_text_emb, *self.depformer_emb], self.linears)

    def depth_frame_tables(self):
        """Pointer tables of the persistent depth-frame launch (``lm.depth_frame.DepthFrameTables``), rebuilt when a weight changes."""
        return self.depth_decoder.tables()

    def depformer_in_all(self) -> torch.Tensor:
        """``[dep_q * depformer_dim, dim]``: the dep_q ``depformer_in[k]`` matrices stacked."""
        return self.depth_decoder.in_all()

    def depformer_in_all_w8(self) -> Optional[tuple]:
        """The ``(q, scale)`` fp8 copy of ``depformer_in_all()`` of a quantised model (rows quantise independently, so stacking the
        per-matrix copies IS the copy of the stacked matrix), or None."""
        if self.weight_dtype == "bf16":
            return None
        pairs = [_w8(m) for m in self.depformer_in]
        if any(c is None for c in pairs):
            return None
        return self._in_cat8.get(tuple(c[0] for c in pairs), lambda: (torch.cat([c[0] for c in pairs], 0).contiguous(),
                                                                     torch.cat([c[1] for c in pairs], 0).contiguous()))

    def _layer_weights(self):
        """(module, parameter name) of the four per-layer matrices of the temporal stack: the ones ``"mxfp4"`` stores as MXFP4."""
        for layer in self.transformer.layers:
            yield layer.self_attn, "in_proj_weight"
            yield layer.self_attn.out_proj, "weight"
            yield layer.gating.linear_in, "weight"
            yield layer.gating.linear_out, "weight"

    def _covered_weights(self):
        """(module, parameter name) of every matrix ``quantize_weights_`` covers."""
        yield from self._layer_weights()
        yield self.text_linear, "weight"
        for m in self.depformer_in:
            yield m, "weight"

    @torch.no_grad()
    def quantize_weights_(self, weight_dtype: str = "fp8", batched: bool = False) -> "LMModel":
        """Weight-only fp8 storage for the decode step at every batch size and for prefill, in place; returns ``self``.  Idempotent.

        Every COVERED matrix -- the temporal transformer's ``in_proj_weight``, ``out_proj.weight``, ``gating.linear_in.weight``,
        ``gating.linear_out.weight``, ``text_linear.weight`` and the ``depformer_in[k]`` (13.5 of the 14.76 GB a Moshi-7B frame
        streams) -- is quantised to e4m3fn bytes with one power-of-two scale per row (``ops.quantize_rows_fp8``), its bf16 parameter is
        OVERWRITTEN with the dequantised values (exact in bf16; also in the tensors of a state dict the model was built from
        without copying), and ``(q, scale)`` stay on the module as non-persistent buffers.  ``state_dict()`` and anything else that
        reads ``.weight`` therefore see the same model as the kernels that stream the fp8 copy: the batch <= 2 GEMVs (``ops.gemv_fp8w``)
        and, above two rows -- the batched step, the many-stream server and pipeline, ``LMGen.prefill`` / ``forward_text(S > 1)`` in
        64-row chunks -- the weight-only fp8 skinny GEMM (``ops.gemm_skinny_fp8w``: K a multiple of 32, else the bf16 parameter), which
        returns what the bf16 route returns on these parameters.  The bf16 copies stay resident; the MFMA-ordered bf16 copies of the
        batched bf16 route are not built for the matrices the fp8 route serves.

        NOT covered, on purpose: embeddings (row lookups, not streams), the depth transformer and the audio heads (they live in
        the persistent depth-frame launch's bf16 pointer tables: 1.27 GB per frame, a separate piece of work) and the norms.
        A quantised model does not take the persistent temporal launch (it reads bf16).

        Captured frame graphs embed weight pointers, so quantising while a streaming session of this model is live raises
        ``RuntimeError``: quantise first, then open the session.  Speech quality under fp8 weights has not been evaluated.

        ``weight_dtype="mxfp4"``: the four per-layer matrices of the temporal stack (6.6 of those GB) are stored as OCP MXFP4 instead
        -- e2m1 codes in blocks of 32 along K with one power-of-two scale byte per block (``ops.quantize_blocks_mxfp4``, buffers
        ``<name>_q4`` / ``<name>_s4``, streamed by ``ops.gemv_mxfp4w`` at batch <= 2; above two rows these matrices are read as bf16 unless ``batched``, below),
        again with the bf16 parameter overwritten by the exactly representable dequantised values; a per-layer matrix whose K is no
        multiple of 32 is stored as fp8.  The two output-facing matrices, ``text_linear`` and the ``depformer_in[k]``, stay at fp8 (and
        take the fp8 skinny GEMM above two rows).  Round-to-nearest MXFP4 has an rms relative weight
        error of 11.5 % on Gaussian rows (fp8: 2.7 %) and speech quality under it has not been evaluated.  Weights with
        ``|w| >= 2^120`` are refused.  A model quantised to one format cannot be quantised to the other: its parameters have
        already been rounded once (``ValueError``).

        ``batched=True`` (``"mxfp4"`` only; opt-in, off by default): the MXFP4 copies are streamed above two rows as well -- the batched
        step, the many-stream server and pipeline, ``LMGen.prefill`` / ``forward_text(S > 1)`` in 64-row chunks -- by the weight-only
        MXFP4 skinny GEMM (``ops.gemm_skinny_mxfp4w``: the codes decoded to the bf16 operand inside the launch, bit for bit what the bf16
        route returns on these parameters, from a quarter of the bytes), and the MFMA-ordered bf16 copies of the batched bf16 route are
        not built for these matrices.  ``mxfp4_batched`` says which route the model takes.  On a model already at ``"mxfp4"`` the call
        only switches the route on (nothing is quantised again; the route stays on once asked for).  With ``"fp8"`` it raises
        ``ValueError``: fp8 copies already serve every batch size."""
        if batched and weight_dtype != "mxfp4":
            raise ValueError(f"batched=True selects the batched route of MXFP4 copies; {weight_dtype!r} copies "
                             + ("already serve every batch size" if weight_dtype == "fp8" else "have none"))
        if weight_dtype == "bf16":
            if self.weight_dtype != "bf16":
                raise ValueError("a quantised model cannot return to bf16: the bf16 parameters already hold the rounded values")
            return self
        if weight_dtype not in ("fp8", "mxfp4"):
            raise ValueError(f"weight_dtype must be 'bf16', 'fp8' or 'mxfp4', got {weight_dtype!r}")
        if self.weight_dtype not in ("bf16", weight_dtype):
            raise ValueError(f"the model is already quantised to {self.weight_dtype!r}: its parameters hold values rounded once and "
                             f"cannot be quantised to {weight_dtype!r}")
        if self._streaming_state is not None or self.transformer._streaming_state is not None:
            raise RuntimeError("quantize_weights_ inside a live streaming session: a captured frame graph would keep streaming the "
                               "bf16 weights; quantise before `streaming()`")
        covered = list(self._covered_weights())
        for mod, name in covered:
            w = getattr(mod, name)
            if w.dtype != torch.bfloat16:
                raise TypeError(f"quantize_weights_ needs bf16 weights, got {w.dtype}")
            if not bool(torch.isfinite(w).all()):
                raise ValueError(f"quantize_weights_: non-finite values in a {tuple(w.shape)} weight; nothing was quantised")
        as_mxfp4 = set()
        if weight_dtype == "mxfp4":
            for mod, name in self._layer_weights():
                w = getattr(mod, name)
                if w.shape[1] % 32 == 0:
                    as_mxfp4.add((id(mod), name))
                    if bool((w.abs() >= 2.0 ** 120).any()):
                        raise ValueError(f"quantize_weights_: magnitudes >= 2^120 in a {tuple(w.shape)} weight; nothing was quantised")
        for mod, name in covered:
            w = getattr(mod, name)
            if (id(mod), name) in as_mxfp4:
                if _w4(mod, name) is None:
                    q, scale = ops.quantize_blocks_mxfp4(w.detach())
                    w.copy_(ops.dequantize_blocks_mxfp4(q, scale))
                    _attach_copy(mod, name, "4", q, scale)
            elif _w8(mod, name) is None:
                q, scale = ops.quantize_rows_fp8(w.detach())
                w.copy_(ops.dequantize_rows_fp8(q, scale))
                _attach_copy(mod, name, "8", q, scale)
        self.weight_dtype = self.transformer.weight_dtype = weight_dtype
        self.mxfp4_batched = self.transformer.mxfp4_batched = self.mxfp4_batched or bool(batched)
        return self

    # ---- token-id conventions (models/model.py:226-277)
    @property
    def initial_token_id(self) -> int:
        return self.card

    @property
    def text_initial_token_id(self) -> int:
        return self.text_card

    @property
    def text_padding_token_id(self) -> int:
        return self.text_card if self.existing_text_padding_id is None else self.existing_text_padding_id

    @property
    def end_of_text_padding_id(self) -> int:
        return 0

    @property
    def zero_token_id(self) -> int:
        return -1

    @property
    def ungenerated_token_id(self) -> int:
        return -2

    @property
    def device(self):
        return next(iter(self.parameters())).device

    @property
    def num_codebooks(self) -> int:
        return self.n_q + 1

    @property
    def num_audio_codebooks(self) -> int:
        return self.n_q

    @property
    def audio_offset(self) -> int:
        return 1

    def _get_initial_token(self) -> torch.Tensor:
        tok = torch.full([1, self.num_codebooks, 1], self.initial_token_id, device=self.device, dtype=torch.long)
        tok[:, 0] = self.text_initial_token_id
        return tok

    @torch.no_grad()
    def forward(self, sequence: torch.Tensor, masks: Optional[torch.Tensor] = None):
        """models/model.py:297-319 (inference only; ``masks`` is unused there too): sequence int64 ``[B, n_q+1, S]`` -> (audio_logits fp32
        ``[B,S,dep_q,card]``, text_logits fp32 ``[B,S,V]``).  The global input is the sequence shifted right behind the initial frame;
        its text ids give the local start token and its first ``dep_q`` audio rows the local sequence."""
        B, K, S = sequence.shape
        shifted = torch.cat([self._get_initial_token().repeat(B, 1, 1), sequence[:, :, :-1]], dim=2)
        transformer_out, text_logits = self.forward_text(shifted)
        audio_logits = self.forward_local(shifted[:, 0, :], shifted[:, 1:self.dep_q + 1, :], transformer_out)
        return audio_logits, text_logits.squeeze(1)

    @torch.no_grad()
    def forward_local(self, local_start_token: torch.Tensor, sequence: torch.Tensor, transformer_out: torch.Tensor) -> torch.Tensor:
        """Teacher-forced depth logits (models/model.py:321-362).  ``local_start_token``: the ``depformer_text_emb`` embedding of the
        text ids, float ``[B,T,depformer_dim]`` as in the reference, or the int64 ids ``[B,T]`` themselves; ``sequence`` int64
        ``[B,dep_q,T]``, ``transformer_out`` fp32 ``[B,T,dim]`` -> ``[B,T,dep_q,card]``.  ``dep_q`` depth steps over ``B*T`` rows on a
        ring of capacity ``dep_q + 1`` (the non-streaming reference path has no ring, hence no Q1 slot quirk at the last codebook)."""
        return self.depth_decoder.forward_local(local_start_token, sequence, transformer_out)

    # ---- decode step / multi-position pass
    def forward_text(self, sequence: torch.Tensor, masks: Optional[torch.Tensor] = None):
        """sequence int64 ``[B, n_q+1, S]`` -> (transformer_out fp32 ``[B,S,dim]``, text_logits fp32 ``[B,1,S,V]``).  ``S == 1``: one
        decode step.  ``S > 1`` inside ``streaming()``: the S positions that follow the ones already streamed, equal to S single steps
        (window ``min(context, capacity - 1)``); outside it: positions 0 .. S-1 under the plain causal + context mask of the
        reference's non-streaming pass (models/model.py:364-389), on throw-away rings of capacity ``S + 1``."""
        B, K, S = sequence.shape
        assert K == self.num_codebooks, f"Sequence shape {sequence.shape} must match the number of codebooks."
        tables = [e.weight for e in self.emb] + [self.text_emb.weight]
        w8 = _w8(self.text_linear) if self.weight_dtype != "bf16" else None
        if S == 1:
            toks = sequence.reshape(B, K).contiguous()
            x = ops.embed_sum(toks, tables, list(range(1, K)) + [0])     # ((e_0 + e_1) + ...) + text, as the reference
            x = self.transformer.step(x)
            out = ops.rmsnorm(x, self.out_norm.alpha_f32(), self.out_norm.eps)
            logits = ops.lm_linear(out, self.text_linear.weight, w8=w8)
            return out.view(B, 1, self.dim), logits.view(B, 1, 1, -1)
        toks = sequence.permute(0, 2, 1).reshape(B * S, K).contiguous()
        x = ops.embed_sum(toks, tables, list(range(1, K)) + [0])
        tr = self.transformer
        saved = tr._streaming_state
        if saved is None:
            tr._streaming_state = tr._init_streaming_state(B, capacity=S + 1)
        try:
            x = tr.run(x, B, S)
        finally:
            tr._streaming_state = saved
        out = ops.rmsnorm(x, self.out_norm.alpha_f32(), self.out_norm.eps)
        logits = ops.lm_linear(out, self.text_linear.weight, w8=w8)
        return out.view(B, S, self.dim), logits.view(B, 1, S, -1)

    def forward_depformer(self, depformer_cb_index: int, sequence: torch.Tensor, transformer_out: torch.Tensor) -> torch.Tensor:
        """sequence int64 ``[B,1,1]`` (previous token), transformer_out fp32 ``[B,1,dim]`` -> logits fp32 ``[B,1,1,card]``."""
        B, K, S = sequence.shape
        assert K == 1, f"Codebooks for Depformer streaming should be passed 1 by 1, got {K}."
        assert S == 1, f"Steps for Depformer streaming should be passed 1 by 1, got {S}."
        assert transformer_out.shape[1] == 1, "Transformer out should be a for a single step."
        logits = self._depformer_logits(depformer_cb_index, sequence.reshape(B, 1).contiguous(), 0,
                                        transformer_out.reshape(B, self.dim).contiguous())
        return logits.view(B, 1, 1, -1)

    def _depformer_logits(self, k: int, tokens: torch.Tensor, col: int, h_t: Optional[torch.Tensor], pos: Optional[torch.Tensor] = None,
                          step_index: Optional[int] = None, h_all: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Depth step ``k``: previous token = ``tokens[:, col]`` (int64 ``[B, n]``), ``h_t`` fp32 ``[B, dim]`` -> logits ``[B, card]``.
        ``h_all`` (``[B, dep_q * depformer_dim]``, the stacked ``depformer_in`` products of the frame) replaces ``h_t``."""
        w8 = _w8(self.depformer_in[k]) if h_all is None and self.weight_dtype != "bf16" else None
        return self.depth_decoder.step_logits(k, tokens, col, h_t, h_all=h_all, w8=w8, pos=pos, step_index=step_index)

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], cfg: dict, kv_dtype: torch.dtype = torch.bfloat16,
                        weight_dtype: str = "bf16", batched: bool = False) -> "LMModel":
        """Model for ``cfg`` (keys of ``rstnet_amd.synth.LM_*``) with weights taken from ``sd`` WITHOUT copying them
        (a 7.7 B-parameter state dict stays a single 15 GB allocation).  ``kv_dtype``: precision of the temporal KV rings.
        ``weight_dtype="fp8"`` / ``"mxfp4"``: ``quantize_weights_`` on the loaded model (it rewrites the covered tensors of ``sd`` in place);
        ``batched``: its keyword (``"mxfp4"`` only: the MXFP4 copies also serve the routes above two rows)."""
        model = cls(kv_dtype=kv_dtype, causal=True, layer_scale=None, gating="silu", norm="rms_norm_f32", positional_embedding="rope",
                    depformer_causal=True, depformer_layer_scale=None, depformer_multi_linear=True, depformer_context=8,
                    depformer_gating="silu", depformer_pos_emb="none", depformer_weights_per_step=True, device="meta", **cfg)
        adopt_state_dict(model, sd)
        return model.eval().quantize_weights_(weight_dtype, batched=batched)


def prefill_token_plan(cache: torch.Tensor, offset: int, user: torch.Tensor, own: torch.Tensor, delays: List[int], initial: torch.Tensor):
    """The token bookkeeping of ``T`` teacher-forced ``LMGen.step`` frames at once (models/model.py:506-521, 545-562), as a pure function
    built from torch indexing (CPU or device tensors): token ring ``cache`` int64 ``[B, K, CT]`` at frame ``offset``, ``user`` ``[B, Ki, T]``,
    ``own`` ``[B, n_own, T]`` (the tokens frame t would have sampled), ``delays`` (K ints), ``initial`` int64 ``[K]`` -> (the model input
    columns ``[B, K, T]``, the ring after the T frames).

    Frame t (o = offset + t) writes user stream k at column o + delay_k, the initial token at column o while o <= delay_k, reads column
    o, then writes ``own[:, :, t]`` at column o + 1.  A column is never more than ``max_delay + 1`` ahead of the frame that writes it, so
    on the UNROLLED axis j = column - offset every write has its own place, later frames write later columns, and the ring ends up
    holding, per stream and slot, the last written column that maps to the slot."""
    B, K, CT = cache.shape
    Ki, T, n_own = user.shape[1], user.shape[2], own.shape[1]
    assert Ki + n_own == K and len(delays) == K and own.shape[2] == T and max(delays) + 2 <= CT
    dev = cache.device
    j = torch.arange(T + CT, device=dev)
    line = cache[:, :, (offset + j) % CT]                    # columns offset .. offset + T + CT - 1 (j < CT: what the ring holds now)
    line[:, :n_own, 1:T + 1] = own
    for q in range(Ki):
        k = n_own + q
        line[:, k, delays[k]:delays[k] + T] = user[:, q]
    for k, d in enumerate(delays):                           # the initial token wins: it is written by the frame that reads the column
        n = min(T, d - offset + 1)
        if n > 0:
            line[:, k, :n] = initial[k]
    # last written column per stream (own streams: offset + T; user streams: offset + T - 1 + delay), and from it the newest column
    # of every slot; a slot whose newest column lies before `offset` was not written and keeps its entry
    last = torch.tensor([T if k < n_own else T - 1 + d for k, d in enumerate(delays)], device=dev).view(K, 1)
    slot = torch.arange(CT, device=dev).view(1, CT)
    newest = last - (offset + last - slot) % CT
    ring = torch.where((newest >= 0).unsqueeze(0), line.gather(2, newest.clamp(min=0).unsqueeze(0).expand(B, K, CT)), cache)
    return line[:, :, :T], ring


SAMPLING_KEYS = ("use_sampling", "temp", "temp_text", "top_k", "top_k_text", "seed")


def check_sampling(values: dict, top_k_cap: int, top_k_text_cap: int) -> dict:
    """One stream's sampling settings as ``set_stream_sampling`` takes them -> the same with every value in its type; ``ValueError`` for an
    unknown key, a temperature that is negative or not finite, a top-k outside ``1 .. cap``, a seed outside ``0 .. 2^64 - 1``.  ``None``
    entries are dropped.  Host arithmetic only (the slot server validates a client's settings with it before the upgrade)."""
    out = {}
    for key, v in values.items():
        if key not in SAMPLING_KEYS:
            raise ValueError(f"unknown sampling setting {key!r} (known: {', '.join(SAMPLING_KEYS)})")
        if v is None:
            continue
        if key == "use_sampling":
            out[key] = bool(v)
        elif key in ("temp", "temp_text"):
            t = float(v)
            if not math.isfinite(t) or t < 0.0:
                raise ValueError(f"{key} = {v!r}: a temperature is a finite number >= 0")
            out[key] = t
        elif key in ("top_k", "top_k_text"):
            cap = top_k_cap if key == "top_k" else top_k_text_cap
            if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= cap:
                raise ValueError(f"{key} = {v!r}: an integer in 1 .. {cap} (the cap is the session's {key})")
            out[key] = int(v)
        else:
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 1 << 64:
                raise ValueError(f"seed = {v!r}: an integer in 0 .. 2^64 - 1")
            out[key] = int(v)
    return out


def _draw_seeds(n: int) -> List[int]:
    """``n`` seeds from torch's default CPU generator (``torch.manual_seed`` makes a run repeatable)."""
    return [int(v) for v in torch.randint(0, 1 << 62, (n,), dtype=torch.int64).tolist()]


class _StreamSampling:
    """Per-stream sampling of a per-stream session: the device tables the frame's samplers and its noise launch read,
    their host mirror, and the persistent noise buffer.  The captured frame holds the tables' addresses; ``write`` updates them in place."""

    def __init__(self, B: int, device, defaults: dict, n_noise: int):
        self.rows = [dict(defaults, seed=s) for s in _draw_seeds(B)]
        self.temp_text = torch.zeros(B, device=device, dtype=torch.float32)
        self.temp = torch.zeros(B, device=device, dtype=torch.float32)
        self.top_k_text = torch.ones(B, device=device, dtype=torch.int32)
        self.top_k = torch.ones(B, device=device, dtype=torch.int32)
        self.seed = torch.zeros(B, device=device, dtype=torch.int64)          # uint64 bit patterns
        self.noise = torch.zeros(B, n_noise, device=device, dtype=torch.float32)
        self.write(("temp", "temp_text", "top_k", "top_k_text", "seed"))

    def write(self, fields) -> None:
        """The named tables from the host mirror: one whole-table copy per table (B values), whatever the number of rows changed."""
        for f in fields:
            if f in ("temp", "temp_text"):
                getattr(self, f).copy_(torch.tensor([r[f] if r["use_sampling"] else 0.0 for r in self.rows], dtype=torch.float32))
            elif f in ("top_k", "top_k_text"):
                getattr(self, f).copy_(torch.tensor([r[f] for r in self.rows], dtype=torch.int32))
            else:
                self.seed.copy_(torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in (r["seed"] for r in self.rows)], dtype=torch.int64))


@dataclass
class _LMGenState:
    cache: torch.Tensor            # int64 [B, K, max_delay + 2] token ring
    initial: torch.Tensor          # int64 [1, K, 1]
    offset_dev: torch.Tensor       # int64 [1]: the frame counter as the ring kernels see it; per-stream session: int64 [B], one per stream
    graphed_frame: _Graphed
    gate: RecaptureGate                    # whether the device's persistent launches were retired since the frame graph was captured
    depth: Optional[_StepState] = None     # the depth transformer's KV rings of THIS session (a captured frame points at them)
    offset: int = 0
    tables: object = None                  # the DepthFrameTables the captured frame points at (kept alive with the graph)
    temporal_base: Optional[int] = None    # host-side position of the temporal rings at frame 0 of this session
    temporal_choice: Optional[bool] = None  # whether the captured frame takes the persistent temporal launch
    frames: Optional[List[int]] = None     # per-stream session: host mirror of `offset_dev`, frames each stream has stepped since its (re)start
    sampling: Optional[_StreamSampling] = None   # LMGen(per_stream_sampling=True) on a per-stream session: the tables the frame samples by

    def reset(self) -> None:
        self.offset = 0
        self.offset_dev.zero_()
        self.temporal_base = None       # (the temporal rings were reset with the session: re-read their position at the next frame)
        if self.frames is not None:
            self.frames = [0] * len(self.frames)


class LMGen(StreamingModule[_LMGenState]):
    """models/model.py:443-597.  The token ring, the delay pattern and the frame counter live on the device
    (csrc/lm_ring.hip), so one frame -- ring update, temporal step, text sample, ``dep_q`` depth steps with their samples,
    ring commit + delayed gather -- is ONE captured graph fed by a single copy of the user tokens."""

    def __init__(self, lm_model: LMModel, use_sampling: bool = True, temp: float = 0.8, temp_text: float = 0.7,
                 top_k: int = 250, top_k_text: int = 25, check: bool = False, per_stream_sampling: bool = False):
        assert not lm_model.training, "generation shouldn't be used in training mode."
        super().__init__()
        self.lm_model = lm_model
        self.use_sampling, self.temp, self.temp_text = use_sampling, temp, temp_text
        self.top_k, self.top_k_text, self.check = top_k, top_k_text, check
        # per_stream_sampling: in a per-stream session every stream samples by its own temperatures, top-k and seed, read
        # from device tables (`set_stream_sampling`); the constructor's values are the defaults, its two top-k the caps
        self.per_stream_sampling = bool(per_stream_sampling)
        if self.per_stream_sampling:
            check_sampling(self.default_sampling(), max(int(top_k), 1), max(int(top_k_text), 1))    # (a top-k <= 0, "all ids", is no cap)
        self.max_delay = max(lm_model.delays)
        self.delays_cuda = torch.tensor(lm_model.delays, device=lm_model.device, dtype=torch.long)
        self._delays_i32 = self.delays_cuda.to(torch.int32)
        self._depth_pos = torch.arange(lm_model.dep_q, device=lm_model.device, dtype=torch.long)

    def _init_streaming_state(self, batch_size: int) -> _LMGenState:
        lm = self.lm_model
        cache = torch.full((batch_size, lm.num_codebooks, self.max_delay + 2), lm.ungenerated_token_id, device=lm.device,
                           dtype=torch.long)
        disable = lm.device.type != "cuda"
        per_stream = self._streaming_per_stream
        sampling = None
        if per_stream and self.per_stream_sampling:
            sampling = _StreamSampling(batch_size, lm.device, self.default_sampling(), self.top_k_text + lm.dep_q * self.top_k)
        return _LMGenState(cache, lm._get_initial_token(), torch.zeros(batch_size if per_stream else 1, device=lm.device, dtype=torch.long),
                           _Graphed(self._frame, disable=disable), RecaptureGate(lm.device),
                           depth=lm.depformer._init_streaming_state(batch_size), frames=[0] * batch_size if per_stream else None,
                           sampling=sampling)

    def default_sampling(self) -> dict:
        """The constructor's sampling settings: what every stream of a ``per_stream_sampling`` session starts with."""
        return dict(use_sampling=bool(self.use_sampling), temp=float(self.temp), temp_text=float(self.temp_text), top_k=int(self.top_k),
                    top_k_text=int(self.top_k_text))

    def _sampling_state(self) -> _StreamSampling:
        state = self._streaming_state
        if state is None:
            raise RuntimeError("You should wrap those calls with a `with lm_gen.streaming(): ...`.")
        if state.sampling is None:
            raise ValueError("per-stream sampling needs LMGen(..., per_stream_sampling=True) and a session opened with "
                             "streaming(batch_size, per_stream=True)")
        return state.sampling

    def set_stream_sampling(self, rows, *, use_sampling=None, temp=None, temp_text=None, top_k=None, top_k_text=None, seed=None) -> None:
        """Streams ``rows`` sample by these settings from the next frame on; ``None`` leaves a setting as it is.  A value holds for every
        row of ``rows``, or is a sequence with one value per row (in the order of ``rows``).  ``top_k`` / ``top_k_text`` lie in 1 .. the
        constructor's value (the cap: it fixes the noise layout, so one stream's top-k moves nobody's draws); a temperature is finite and
        >= 0 (0: greedy); ``use_sampling=False`` makes the stream greedy and keeps its temperatures for a later ``True``; ``seed``
        (0 .. 2^64 - 1) starts the stream's noise over as ``(seed, its own frame counter)``.  Everything is validated on the host before
        anything is written; the writes are eager in-place copies between two frames, like ``reset_streams``: the captured frame reads the
        tables from device memory and stays valid."""
        sp = self._sampling_state()
        order = [int(b) for b in rows]
        check_rows(order, len(sp.rows))
        if len(set(order)) != len(order):
            raise ValueError(f"set_stream_sampling: rows {order} name a stream twice")
        given = dict(use_sampling=use_sampling, temp=temp, temp_text=temp_text, top_k=top_k, top_k_text=top_k_text, seed=seed)
        new = [dict() for _ in order]
        for key, v in given.items():
            if v is None:
                continue
            vals = list(v) if isinstance(v, (list, tuple)) else [v] * len(order)
            if len(vals) != len(order):
                raise ValueError(f"set_stream_sampling: {key} has {len(vals)} values for {len(order)} rows")
            for d, x in zip(new, vals):
                d[key] = x
        cap, cap_text = max(int(self.top_k), 1), max(int(self.top_k_text), 1)
        new = [check_sampling(d, cap, cap_text) for d in new]
        touched = set()
        for b, d in zip(order, new):
            sp.rows[b].update(d)
            touched |= set(d)
        if "use_sampling" in touched:
            touched |= {"temp", "temp_text"}
        sp.write(sorted(touched - {"use_sampling"}))

    def stream_sampling(self, b: int) -> dict:
        """Stream ``b``'s sampling settings (from the host mirror of the device tables)."""
        sp = self._sampling_state()
        (b,) = check_rows([b], len(sp.rows))
        return dict(sp.rows[b])

    def reset_streams(self, rows) -> None:
        """Streams ``rows`` of a per-stream session (``streaming(batch_size, per_stream=True)``) start a new conversation with the next
        frame: their token-ring rows go back to ``ungenerated_token_id``, their frame counters and their positions on the temporal rings
        to 0.  The other streams do not notice.  Eager in-place writes between two frames: the captured frame reads all three from device
        memory and stays valid.  ``step`` output of such a stream is meaningful again once ``stream_valid()`` lists it."""
        state = self._streaming_state
        if state is None:
            raise RuntimeError("You should wrap those calls with a `with lm_gen.streaming(): ...`.")
        if state.frames is None:
            raise ValueError("reset_streams needs a per-stream session: open it with streaming(batch_size, per_stream=True)")
        rows = check_rows(rows, len(state.frames))
        if not rows:
            return
        lm = self.lm_model
        state.cache[rows] = lm.ungenerated_token_id
        state.offset_dev[rows] = 0
        tst = lm.transformer._streaming_state
        if tst is not None:
            if not tst.per_stream:
                raise ValueError("reset_streams: the model's temporal rings keep one position for the batch (the session was not opened per stream)")
            tst.pos[rows] = 0
        for b in rows:
            state.frames[b] = 0
        if state.sampling is not None:
            # a new conversation draws a new seed (default CPU generator); its settings stay until set_stream_sampling changes them
            for b, s in zip(rows, _draw_seeds(len(rows))):
                state.sampling.rows[b]["seed"] = s
            state.sampling.write(("seed",))

    def stream_valid(self) -> List[int]:
        """The streams whose last ``step`` output is meaningful: those whose own frame count exceeds ``max_delay`` (a scalar session:
        all of them or none)."""
        state = self._streaming_state
        if state is None:
            raise RuntimeError("You should wrap those calls with a `with lm_gen.streaming(): ...`.")
        if state.frames is None:
            B = state.cache.shape[0]
            return list(range(B)) if state.offset > self.max_delay else []
        return [b for b, n in enumerate(state.frames) if n > self.max_delay]

    def _noise(self, B: int, k: int) -> Optional[torch.Tensor]:
        if not self.use_sampling:
            return None
        return torch.empty(B, k, device=self.lm_model.device, dtype=torch.float32).exponential_(1)   # utils/sampling.py:44

    def _frame(self, user_tokens: torch.Tensor):
        """user_tokens int64 ``[B, Ki]`` -> (delay-aligned output ``[B, dep_q + 1]``, model input ``[B, K]``); everything in
        between stays on the device (this is the function that is captured)."""
        state, lm = self._streaming_state, self.lm_model
        B = user_tokens.shape[0]
        input_ = ops.lm_ring_begin(state.cache, user_tokens, state.initial.reshape(-1), self._delays_i32, state.offset_dev,
                                   lm.dep_q + 1)
        # one draw of Exp(1) noise per frame for the text sampler and the dep_q audio samplers (utils/sampling.py:44-46)
        sp = state.sampling
        if sp is not None:
            # per-stream sampling: the same columns (text, then dep_q blocks of top_k) from each stream's own (seed, frame counter) stream,
            # read here, before lm_ring_commit moves the counters
            noise = ops.noise_exp_rows(sp.seed, state.offset_dev, sp.noise.shape[1], out=sp.noise)
        else:
            noise = self._noise(B, self.top_k_text + lm.dep_q * self.top_k)
        transformer_out, text_logits = lm.forward_text(input_.view(B, -1, 1))
        tokens = torch.empty(B, lm.dep_q + 1, device=input_.device, dtype=torch.long)
        if sp is not None:
            ops.lm_sample_ps(text_logits.view(B, -1), top_k=self.top_k_text, noise=noise[:, :self.top_k_text], temps=sp.temp_text,
                             top_ks=sp.top_k_text, out=tokens[:, 0])
        else:
            ops.lm_sample(text_logits.view(B, -1), use_sampling=self.use_sampling, temp=self.temp_text, top_k=self.top_k_text,
                          noise=None if noise is None else noise[:, :self.top_k_text], out=tokens[:, 0])
        self._depth(tokens, transformer_out.view(B, lm.dim).contiguous(), None if noise is None else noise[:, self.top_k_text:], sp)
        out = ops.lm_ring_commit(state.cache, tokens, self._delays_i32, state.offset_dev, self.max_delay)
        return out, input_

    def _depth(self, tokens: torch.Tensor, h_t: torch.Tensor, noise: Optional[torch.Tensor], sp: Optional[_StreamSampling] = None) -> None:
        """The ``dep_q`` sequential depth-transformer steps (models/model.py:564-597): ``tokens[:, 0]`` is the text token,
        step ``cb`` embeds ``tokens[:, cb]`` and samples ``tokens[:, cb + 1]`` in place.  The depth KV rings are persistent
        buffers; the steps are positions 0 .. dep_q - 1 of a ring that restarts every frame (= the reference's fresh
        ``with depformer.streaming(B)`` context), supplied as constant device scalars instead of a counter to reset and bump."""
        B, lm, state = tokens.shape[0], self.lm_model, self._streaming_state
        # the chain's rings belong to the session (so that a frame graph captured by another live session keeps valid pointers and
        # exiting `streaming()` releases them); a bare `depformer_step` call outside any session gets throw-away rings
        mine = state is not None and state.depth is not None and state.depth.k[0].shape[0] == B
        # (``sp``, the session's per-stream sampling tables: the persistent launch keeps scalar parameters, so the chain runs at every batch size)
        lm.depth_decoder.decode_frame(
            tokens, h_t, noise, self._depth_pos, use_sampling=self.use_sampling, temp=self.temp, top_k=self.top_k, keep=state,
            rings=state.depth if mine else lm.depformer._init_streaming_state, w8=lm.depformer_in_all_w8(),
            persistent=h_t.is_cuda and sp is None, temps=None if sp is None else sp.temp, top_ks=None if sp is None else sp.top_k)

    @torch.no_grad()
    def step(self, input_tokens: torch.Tensor) -> Optional[torch.Tensor]:
        state = self._streaming_state
        if state is None:
            raise RuntimeError("You should wrap those calls with a `with lm_gen.streaming(): ...`.")
        lm = self.lm_model
        assert input_tokens.dim() == 3, "Shape should be [B, K, T]."
        B, Ki, S = input_tokens.shape
        assert S == 1, "Only support being given steps one by one."
        needed = lm.num_codebooks - lm.dep_q - 1
        assert Ki == needed, f"We expect {needed} tokens from the user stream, got {Ki}."
        if lm.device.type == "cuda" and state.gate.moved(state.offset):
            # a device that had to repair frames moves to the launch-per-op chain, which needs a fresh capture
            state.graphed_frame = _Graphed(self._frame)
        if state.frames is not None:
            # per-stream session: the streams stand at different frames and positions, all of them on the device (no host mirror of the
            # temporal rings, one route -- ROUTE_DECODE -- at every fill level, so nothing is ever re-captured for a position)
            out, input_ = state.graphed_frame(input_tokens.reshape(B, Ki).contiguous())
            if self.check:
                lm.depth_decoder.check()
            state.offset += 1
            state.frames = [n + 1 for n in state.frames]
            if max(state.frames) <= self.max_delay:
                return None
            return out.view(B, lm.dep_q + 1, 1).clone()
        tst = lm.transformer._streaming_state
        if tst is not None:
            # the temporal rings' fill as the host knows it (graph replays do not run the Python that counts steps): the persistent
            # temporal launch is chosen by it (ops.temporal_frame_wanted), and a frame captured under the other choice is re-captured
            if state.temporal_base is None:
                state.temporal_base = tst.offset_cpu - state.offset
            tst.offset_cpu = state.temporal_base + state.offset
            # (a quantised model never takes it -- _persistent_step -- so its frame is not re-captured when the rings pass that mark)
            want = B == 1 and lm.weight_dtype == "bf16" and ops.temporal_frame_wanted(tst.offset_cpu)
            if state.temporal_choice is None:
                state.temporal_choice = want
            elif want != state.temporal_choice:
                state.temporal_choice = want
                state.graphed_frame = _Graphed(self._frame)
        out, input_ = state.graphed_frame(input_tokens.reshape(B, Ki).contiguous())
        if tst is not None:
            tst.offset_cpu = state.temporal_base + state.offset + 1
        if self.check:
            lm.depth_decoder.check()       # a timed-out hand-off of the persistent depth launch
            assert not (input_ == lm.ungenerated_token_id).any(), (state.offset, input_)
            assert (input_[:, lm.audio_offset:] <= lm.card).all(), input_
            assert (input_[:, :1] <= lm.text_card).all()
        state.offset += 1
        if state.offset <= self.max_delay:
            return None
        return out.view(B, lm.dep_q + 1, 1).clone()

    def model_time(self, outputs: torch.Tensor) -> torch.Tensor:
        """The delay-aligned stream ``step`` returns, ``[B, dep_q + 1, A]`` (A consecutive frames from the first non-None one), as
        model-time frames for ``prefill``: ``model[k][t] = aligned[k][t - delay_k]`` for ``t >= delay_k``; the earlier entries are never
        read (``step`` overwrites their ring columns with the initial token) and hold the initial token."""
        lm = self.lm_model
        B, n, A = outputs.shape
        assert n == lm.dep_q + 1, f"We expect {lm.dep_q + 1} generated streams, got {n}."
        own = lm._get_initial_token().to(outputs.device)[:, :n].repeat(B, 1, A)
        for k, d in enumerate(lm.delays[:n]):
            if d < A:
                own[:, k, d:] = outputs[:, k, :A - d]
        return own

    @torch.no_grad()
    def prefill(self, user_tokens: torch.Tensor, own_tokens: torch.Tensor) -> None:
        """Takes in ``T`` frames that already exist: equal to ``T`` calls of ``step(user_tokens[..., t:t+1])`` in which the tokens frame
        ``t`` sampled (text, then ``dep_q`` audio, in model time: what ``step`` writes to the token ring at ``offset + 1``) are replaced
        by ``own_tokens[..., t]``.  user_tokens int64 ``[B, Ki, T]``, own_tokens int64 ``[B, dep_q + 1, T]`` (``model_time`` builds it
        from recorded ``step`` outputs).  The depth transformer, the output norm and the text head never run; the temporal pass is one
        ``StreamingTransformer.run``.  Works at any session offset; a captured frame graph stays valid (it reads positions from device
        scalars)."""
        state = self._streaming_state
        if state is None:
            raise RuntimeError("You should wrap those calls with a `with lm_gen.streaming(): ...`.")
        if state.frames is not None:
            raise ValueError("LMGen.prefill on a per-stream session: its token plan counts one frame offset for the batch")
        lm = self.lm_model
        assert user_tokens.dim() == 3 and own_tokens.dim() == 3, "Shape should be [B, K, T]."
        B, Ki, T = user_tokens.shape
        needed = lm.num_codebooks - lm.dep_q - 1
        assert Ki == needed, f"We expect {needed} tokens from the user stream, got {Ki}."
        assert own_tokens.shape == (B, lm.dep_q + 1, T), f"We expect own tokens [{B}, {lm.dep_q + 1}, {T}], got {tuple(own_tokens.shape)}."
        if T == 0:
            return
        tst = lm.transformer._streaming_state
        if tst is None:
            raise RuntimeError("LMGen.prefill needs the model's streaming state: open `lm_gen.streaming()` (it propagates to the model)")
        if state.temporal_base is None:
            state.temporal_base = tst.offset_cpu - state.offset
        tst.offset_cpu = state.temporal_base + state.offset      # (graph replays of `step` do not run the Python that counts steps)
        inputs, ring = prefill_token_plan(state.cache, state.offset, user_tokens.to(state.cache.device), own_tokens.to(state.cache.device),
                                          lm.delays, state.initial.reshape(-1))
        K = lm.num_codebooks
        toks = inputs.permute(0, 2, 1).reshape(B * T, K).contiguous()
        tables = [e.weight for e in lm.emb] + [lm.text_emb.weight]
        lm.transformer.run(ops.embed_sum(toks, tables, list(range(1, K)) + [0]), B, T)      # advances pos / offset_cpu by T
        state.cache.copy_(ring)
        state.offset += T
        state.offset_dev.add_(T)

    def depformer_step(self, text_token: torch.Tensor, transformer_out: torch.Tensor) -> torch.Tensor:
        """text_token int64 ``[B]``, transformer_out fp32 ``[B, 1, dim]`` -> the frame's ``dep_q`` audio tokens ``[B, dep_q]``
        (models/model.py:564-597)."""
        (B,) = text_token.shape
        lm = self.lm_model
        tokens = torch.empty(B, lm.dep_q + 1, device=text_token.device, dtype=torch.long)
        tokens[:, 0] = text_token
        self._depth(tokens, transformer_out.reshape(B, lm.dim).contiguous(), self._noise(B, lm.dep_q * self.top_k))
        return tokens[:, 1:]
