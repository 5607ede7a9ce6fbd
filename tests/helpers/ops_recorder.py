"""Recording stand-ins for the ``rstnet_amd.ops`` entry points the LM depth phase and temporal pass call, so that their HOST logic -- which launches it
asks for, on which tensors, with which scalars -- runs and can be compared on CPU tensors.  Every stand-in binds its arguments to the
real entry point's signature (defaults filled in: an omitted keyword and its default are the same request), writes one line to the log
and returns zero tensors of the shape the real launch returns."""
import inspect

import torch

_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int64: "i64", torch.int32: "i32", torch.uint8: "u8"}


def describe(v):
    """A tensor as dtype, shape, strides and storage offset; containers element-wise; pointer tables by what they were built for."""
    if isinstance(v, torch.Tensor):
        return f"{_DT.get(v.dtype, v.dtype)}{list(v.shape)}s{list(v.stride())}+{v.storage_offset()}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(describe(e) for e in v) + "]"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {describe(e)}" for k, e in v.items()) + "}"
    if isinstance(v, torch.device):
        return str(v)
    if hasattr(v, "head_bias") and hasattr(v, "emb_rows"):      # lm.depth_frame.DepthFrameTables
        return (f"tables(L={v.L}, dep_q={v.dep_q}, E={v.E}, H={v.H}, Hd={v.Hd}, card={v.card}, bias={v.head_bias is not None}, "
                f"emb_rows={list(v.emb_rows)}, eps={v.eps}, context={v.context})")
    return repr(v)


class OpsRecorder:
    """``install(monkeypatch, ops)`` replaces the entry points; ``log`` is the list of recorded lines.  ``depth_frame``: the answer of
    ``depth_frame_enabled``; ``epoch``: the answer of ``persistent_epoch``; ``temporal_frame``: the answer of ``temporal_frame_wanted``.
    ``install(..., temporal=True)`` also replaces the entry points only the temporal pass calls."""

    def __init__(self, depth_frame: bool = True, temporal_frame: bool = False):
        self.log, self.depth_frame, self.epoch, self.temporal_frame = [], depth_frame, 0, temporal_frame

    def _record(self, name, real, args, kwargs):
        bound = inspect.signature(real).bind(*args, **kwargs)
        bound.apply_defaults()
        a = dict(bound.arguments)
        if name == "depth_decode_frame":        # the effective ring capacity (ops.depth_decode_frame: default = the tables' dep_q)
            a["ring_cap"] = a["ring_cap"] or a["tables"].dep_q
        self.log.append(f"{name}(" + ", ".join(f"{k}={describe(v)}" for k, v in a.items()) + ")")
        return a

    def install(self, monkeypatch, ops, temporal: bool = False) -> "OpsRecorder":
        f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32)
        rec = self

        class TemporalTables:      # stands for ops.TemporalFrameTables: no pointers, only what it was built for
            def __init__(self, layers, *, H, context, eps):
                self.text = f"temporal_tables(L={len(layers)}, H={H}, context={context}, eps={eps})"
                rec.log.append(f"TemporalFrameTables(layers={describe(list(layers))}, H={H}, context={context}, eps={eps})")

            def __repr__(self):
                return self.text
        outputs = {
            "lm_linear": lambda a: f32(a["x"].shape[0], a["w"].shape[0]),
            "gemv_embed": lambda a: (f32(a["add"].shape[0], a["w"].shape[0]), f32(*a["add"].shape)),
            "embed_sum": lambda a: f32(a["tokens"].shape[0], a["tables"][0].shape[1]),
            "gemv_attn": lambda a: f32(a["qkv"].shape[0], a["w"].shape[0]),
            "gemv_attn_supported": lambda a: a["B"] <= 2 and a["cap"] <= 8 and not a["rope"],
            "lm_attn_decode": lambda a: f32(a["qkv"].shape[0], (a["heads"] or a["k_cache"].shape[1]) * a["k_cache"].shape[3]),
            "lm_gated_pair": lambda a: f32(*a["x"].shape),
            "lm_sample": lambda a: a["out"] if a["out"] is not None else torch.zeros(a["logits"].shape[0], dtype=torch.long),
            "depth_frame_enabled": lambda a: self.depth_frame,
            "depth_frame_supported": lambda a: 1 <= a["B"] <= 2,
            "depth_decode_frame": lambda a: None,
            "persistent_epoch": lambda a: self.epoch,
            "persistent_poll": lambda a: None,
            "new_persistent_status": lambda a: torch.zeros(4, dtype=torch.int32),
        }
        if temporal:
            H_D = lambda a: (a["heads"] or a["k_cache"].shape[1]) * a["k_cache"].shape[3]
            outputs.update({
                "lm_rope_append": lambda a: f32(a["qkv"].shape[0], a["heads"], a["qkv"].shape[1], a["k_cache"].shape[3]),
                "attention": lambda a: f32(a["q"].shape[0], a["q"].shape[2], a["q"].shape[1] * a["q"].shape[3]),
                "lm_attn_prefill": lambda a: f32(a["qkv"].shape[0] * a["qkv"].shape[1], H_D(a)),
                "lm_ring_append": lambda a: None,
                "rmsnorm": lambda a: f32(*a["x"].shape),
                "lm_rope_table": lambda a: f32(a["D"] // 2, 2),
                "temporal_frame_wanted": lambda a: self.temporal_frame,
                "temporal_frame_supported": lambda a: a["B"] == 1,
                "temporal_decode_frame": lambda a: f32(*a["x"].shape),
            })
            monkeypatch.setattr(ops, "TemporalFrameTables", TemporalTables)
        for name, out in outputs.items():
            real = getattr(ops, name)
            monkeypatch.setattr(ops, name, lambda *args, _n=name, _r=real, _o=out, **kw: _o(self._record(_n, _r, args, kw)))
        return self
