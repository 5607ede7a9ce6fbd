"""Tensor-level front of the C ABI: PyTorch is used for device memory and streams only.

Every function takes / returns CUDA (HIP) fp32 tensors in the CHANNELS-LAST layout ``[B, T, C]`` unless
stated otherwise, launches on the current stream OF THE DEVICE THE TENSORS LIVE ON (every public function runs under a
device guard for its first tensor argument, so a process may drive ``cuda:N`` without making it the current device) and raises
if handed CPU tensors -- there is no host fallback.

Scratch (split-K partials + arrival counters, attention split workspaces, packed operand buffers, RVQ atomic keys) is cached
per (device, STREAM, shape): launches on one stream are ordered, so layers of equal shape share a buffer; work issued on another
stream gets its own.  A captured graph owns the buffers of its capture stream -- replays of graphs captured on the same stream
must not overlap each other (the server and the pipelines run one session at a time, as the reference's lock does).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from .persistent import (_persist_off, _persist_pending, _persist_status, depth_frame_enabled, new_persistent_status,  # noqa: F401
                         persistent_epoch, persistent_poll, persistent_rearm, persistent_repairs, persistent_retired)
from .slots import record_stride       # bytes between the records of a packed frame buffer (the layouts live in slots.py)

ACT_NONE, ACT_ELU, ACT_GELU = 0, 1, 1   # act_in: 1 = ELU ; act_out: 1 = GELU
ACT_ELU_OUT = 2                          # act_out: ELU applied last (after the residual)
PAD_ZERO, PAD_REPLICATE = 0, 1


# Optional per-launch instrumentation (bench.py's roofline leg): a list that receives
# (kernel name, start event, end event, algorithmic flops, algorithmic bytes) for every GEMM launch.
PROFILE = None


class _profiled:
    """``with _profiled(name, flops, nbytes, shape):`` around the launches of one profile row.  ``PROFILE`` is read once, on entry:
    the row ``(name, start event, end event, flops, nbytes, shape)`` goes to the list it named then, and with ``PROFILE is None``
    no event is created.  A block that raises appends nothing."""
    __slots__ = ("row", "prof", "e0", "e1")

    def __init__(self, name: str, flops: float, nbytes: int, shape: tuple):
        self.row = (name, flops, nbytes, shape)

    def __enter__(self):
        self.prof = PROFILE
        if self.prof is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, exc_type, exc, tb):
        if self.prof is not None and exc_type is None:
            self.e1.record()
            name, flops, nbytes, shape = self.row
            self.prof.append((name, self.e0, self.e1, flops, nbytes, shape))
        return False


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ctx(context: Optional[int]) -> int:
    """Attention context as the library takes it: 0 = unlimited."""
    return int(context) if context else 0


def _first_tensor(args):
    for a in args:
        if isinstance(a, torch.Tensor):
            return a
        if isinstance(a, (tuple, list)) and a and isinstance(a[0], torch.Tensor):
            return a[0]
    return None


def _on_tensor_device(fn):
    """Device guard: run ``fn`` with the device of its first tensor argument current, so that ``_stream()``, the scratch
    allocations and the launch itself all address that device (a tool driving ``cuda:3`` need not call ``set_device``)."""
    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        t = _first_tensor(args)
        if t is not None and t.is_cuda and t.device.index != torch.cuda.current_device():
            with torch.cuda.device(t.device):
                return fn(*args, **kwargs)
        return fn(*args, **kwargs)
    return guarded


class _PackedWeights:
    """Cache of device-side re-packed copies of weight tensors, keyed by (device, address, shape).  An entry dies with the
    STORAGE of its source (weak reference): per-step slices of a parameter are fresh tensor objects on every call but share
    the parameter's storage, and an address that the allocator hands out again after a free can never hit a stale entry.
    A changed ``_version`` (in-place update of the weights) re-packs; so does one of ``also``, the companion tensors (or None) that
    ``build`` packs into the same copy."""

    def __init__(self):
        self._d: dict = {}

    def get(self, w: torch.Tensor, build, also: tuple = ()):
        from torch.multiprocessing.reductions import StorageWeakRef
        key = (w.device, w.data_ptr(), tuple(w.shape), w.dtype)
        versions = (w._version, *(None if t is None else t._version for t in also))
        hit = self._d.get(key)
        if hit is not None and hit[1] == versions and not hit[2].expired():
            return hit[0]
        if len(self._d) > 64:
            for k in [k for k, v in self._d.items() if v[2].expired()]:
                del self._d[k]
        packed = build()
        self._d[key] = (packed, versions, StorageWeakRef(w.untyped_storage()))
        return packed

    def clear(self) -> None:
        self._d.clear()


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr() if t.numel() > 0 else None


def _chk(t: Optional[torch.Tensor], name: str, dtype=torch.float32, contiguous: bool = True) -> None:
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"rstnet_amd.ops: `{name}` is on {t.device}; the HIP path needs a CUDA/HIP tensor (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"rstnet_amd.ops: `{name}` must be {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"rstnet_amd.ops: `{name}` must be contiguous")


def _shared_pos(pos_dev: Optional[torch.Tensor], op: str) -> None:
    """Kernels outside the GPT global transformer know ONE position per call: a per-stream vector is refused, never read as its row 0."""
    if pos_dev is not None and pos_dev.numel() != 1:
        raise ValueError(f"rstnet_amd.ops: {op} takes one position for all streams (numel 1), got {tuple(pos_dev.shape)}; per-stream positions "
                         "are served by lm_attn_decode / lm_rope_table / lm_attn_prefill / lm_ring_append")


def _pos_stride(pos_dev: torch.Tensor, B: int, op: str) -> int:
    """0: ``pos_dev`` holds one position shared by the ``B`` streams (today's entry points); 1: int64 ``[B]``, one per stream."""
    n = pos_dev.numel()
    if n != 1 and (n != B or pos_dev.dim() != 1):
        raise ValueError(f"rstnet_amd.ops: {op}: pos_dev holds one position, or one per stream as int64 [{B}]; got {tuple(pos_dev.shape)}")
    return 0 if n == 1 else 1


_gemm_scratch: dict = {}


def _scratch(cache: dict, device, shape_key: tuple, build):
    """Per-(device, stream, shape) scratch with a twin for graph capture.  A buffer that is first allocated INSIDE a capture is
    zero-filled by a node of the graph, i.e. by one more launch on every replay (measured: 19 such fills per codec frame); so the
    first eager use of a shape also creates the entry captures will look up (key "graph": all captured graphs of a device share
    it -- their replays must not overlap, see the module docstring)."""
    capturing = torch.cuda.is_current_stream_capturing()
    key = (device, "graph" if capturing else _stream()) + shape_key
    sc = cache.get(key)
    if sc is None:
        sc = cache[key] = build()
        if not capturing and (device, "graph") + shape_key not in cache:
            cache[(device, "graph") + shape_key] = build()
    return sc


# K split of the medium-row GEMMs across workgroups: None = rst_gemm_win_split_plan; an int overrides it (probes / A/B runs only)
GEMM_WIN_SPLIT = None


def _split_scratch(device, shape_key: tuple, plan, rows: int, N: int, counters):
    """Split-K plan + scratch of one GEMM shape, ``(split, partials [split, rows, N] fp32, arrival counters int32)`` or
    ``(1, None, None)``, cached per (stream, shape); launches on one stream are ordered and the counters re-arm themselves (zero
    once), so layers of equal shape share the buffers.  ``plan`` / ``counters``: callables, asked when the entry is built."""
    def build():
        sk = int(plan())
        if sk > 1:
            return (sk, torch.empty(sk, rows, N, device=device, dtype=torch.float32),
                    torch.zeros(int(counters()), device=device, dtype=torch.int32))
        return (1, None, None)
    return _scratch(_gemm_scratch, device, shape_key, build)


def _gemm_split_scratch(device, M: int, N: int, K: int):
    """The K split of the medium-row (streaming step) GEMMs."""
    if M > 4096 or M == 0:
        return 1, None, None
    return _split_scratch(device, ("gemm_win", M, N, K, GEMM_WIN_SPLIT),
                          lambda: _lib.lib().rst_gemm_win_split_plan(M, N, K) if GEMM_WIN_SPLIT is None else GEMM_WIN_SPLIT, M, N,
                          lambda: _lib.lib().rst_gemm_win_split_tiles(M, N))


_skinny_f32_weights = _PackedWeights()
SKINNY_F32_MAX_ROWS = 128

# Large launches (more than 4096 rows, N > 64, K % 64 == 0 -- the batched encode / decode of utterances) run on the bf16 matrix
# instruction with every fp32 operand split into three bf16 planes (rst_gemm_win_b3_f32: six products per fp32 product, fp32
# accuracy, 2.7x the f32 instruction's rate).  False: the f32 matrix instruction everywhere (the A/B switch of tools/ab.py).
GEMM_B3 = True
# End-to-end streaming (pipeline.StreamingPipeline): encode -> LM frame -> decode as ONE captured graph per frame once the delay line is
# full.  False: the three module calls with their own graphs (the A/B switch of tools/ab.py).
PIPELINE_FUSE = True
_b3_weights = _PackedWeights()


@_on_tensor_device
def gemm_win_b3_pack_weight(w: torch.Tensor) -> torch.Tensor:
    """fp32 ``[N, K]`` -> its three bf16 planes in the operand order of the large-M kernel (rst_gemm_win_b3_pack_weight), cached per
    storage / version like the other packed copies."""
    _chk(w, "w")
    N, K = w.shape

    def build():
        n = int(_lib.lib().rst_gemm_win_b3_weight_elems(N, K))
        if n <= 0:
            raise ValueError(f"rstnet_amd.ops: no three-plane form for a [{N}, {K}] weight")
        w3 = torch.empty(n, device=w.device, dtype=torch.int16)
        _lib.check(_lib.lib().rst_gemm_win_b3_pack_weight(_ptr(w), _ptr(w3), N, K, _stream()))
        return w3
    return _b3_weights.get(w, build)


def _b3_shape(M: int, N: int, K: int) -> bool:
    return GEMM_B3 and M > 4096 and N > 64 and K % 64 == 0


@functools.lru_cache(maxsize=1024)
def _b3_supported(B: int, T_in: int, T_out: int, C_: int, K: int, N: int, S: int, P: int, pad_mode: int, x_bstride: int, has_hist: bool) -> bool:
    return bool(_lib.lib().rst_gemm_win_b3_supported(B, T_in, T_out, C_, K, N, S, P, pad_mode, x_bstride, int(has_hist)))


def _b3_route(x, hist, w, B: int, T_in: int, T_out: int, C_: int, K: int, N: int, S: int, P: int, pad_mode: int) -> bool:
    """True when this launch runs on the three-plane bf16 kernel: the LIBRARY's predicate (rst_gemm_win_b3_supported: shape, padding,
    4 GB buffer-offset reach) plus 16-byte-aligned operands -- rst_gemm_win_b3_f32 refuses everything else, so a profile row labelled
    `gemm_win_b3` names the kernel that ran."""
    if not GEMM_B3 or not _b3_shape(B * T_out, N, K):
        return False
    if x.data_ptr() % 16 or w.data_ptr() % 16:
        return False
    return _b3_supported(B, T_in, T_out, C_, K, N, S, P, pad_mode, T_in * C_, hist is not None)


@_on_tensor_device
def skinny_f32_pack_weight(w: torch.Tensor) -> torch.Tensor:
    """fp32 ``[N, K]`` -> MFMA-ordered copy ``[ceil(N/32)*32, ceil(K/8)*8]`` (rst_skinny_f32_pack_weight), cached per storage."""
    _chk(w, "w")
    N, K = w.shape

    def build():
        wp = torch.empty((N + 31) // 32 * 32, (K + 7) // 8 * 8, device=w.device, dtype=torch.float32)
        _lib.check(_lib.lib().rst_skinny_f32_pack_weight(_ptr(w), _ptr(wp), N, K, _stream()))
        return wp
    return _skinny_f32_weights.get(w, build)


# K split of the few-row GEMMs across workgroups: None = rst_skinny_f32_split_plan; an int overrides it (probes / A/B runs only)
SKINNY_F32_SPLIT = None

# Plain few-row linears WITHOUT a LayerNorm in front (no window) read their rows row-major inside the GEMM (rst_linear_few_rows_f32): no
# packing launch, the same bits.  False: pack, then the GEMM on the packed operand (the A/B switch of tools/probes/few_row_linear_probe.py).
# (With a LayerNorm the packing launch stays: applying it inside the GEMM was built twice and measured slower, csrc/skinny_f32.hip.)
SKINNY_F32_ROWS = True

# LayerNorm in front of a few-row linear (streamed transformer layers at more than two streams): applied by the packing launch
# (rst_skinny_f32_pack_ln) instead of a launch of its own.  False: LayerNorm, then pack (the A/B switch of tools/ab.py).
SKINNY_F32_PACK_LN = True


class PackedRows:
    """The result of a few-row linear kept in the packed operand order of the NEXT few-row linear (``ops.linear(..., out_packed=True)``):
    ``xp [32 | 64 | 128, N]`` fp32 as rst_skinny_f32_pack_win lays rows out, ``shape`` the logical ``[..., N]``.  Only ``ops.linear``
    consumes it."""

    def __init__(self, xp: torch.Tensor, shape: tuple):
        self.xp, self.shape = xp, tuple(shape)

    def contiguous(self):
        return self


def _packed_row_count(M: int) -> int:
    """Rows of the packed operand of ``M <= 128`` logical rows: every producer and consumer of a ``PackedRows`` pads alike."""
    return 32 if M <= 32 else (64 if M <= 64 else 128)


# linear1 -> GELU -> linear2 of a streamed transformer layer (few-row route): linear1 writes the operand of linear2 in packed order,
# no packing launch between them.  False: row-major result + pack (the A/B switch of tools/ab.py).
SKINNY_F32_CHAIN = True


def linear_chains(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> bool:
    """True when ``ops.linear(x, w1, out_packed=True)`` may feed ``ops.linear(., w2)``: both on the few-row skinny route."""
    K = x.shape[-1]
    M = x.numel() // K if K else 0
    return bool(SKINNY_F32_CHAIN and x.is_cuda and M > 4 and _few_rows(M, w1.shape[0], K) and _few_rows(M, w2.shape[0], w1.shape[0])
                and w1.shape[0] % 8 == 0 and w2.shape[1] == w1.shape[0])


def _gemm_few_rows(x, hist, w, bias, res, scale, out, B, T_in, T_out, C_, K, N, S, P, pad_mode, act_in, act_out, ln=None,
                   out_packed: bool = False) -> None:
    """The streaming-step route of gemm_win / linear: gather + pack the activation windows, then the few-row fp32 skinny GEMM.
    ``ln = (gamma, beta, eps)`` (plain linears only): the LayerNorm of the rows, applied while they are packed.  ``x`` may be a
    ``PackedRows`` (no packing at all); ``out_packed``: ``out`` is the ``xp`` of a ``PackedRows``."""
    M = B * T_out
    wp = skinny_f32_pack_weight(w)
    packed_in = isinstance(x, PackedRows)
    sc = _split_scratch(x.xp.device if packed_in else x.device, ("skinny", M, N, K, SKINNY_F32_SPLIT),
                        lambda: _lib.lib().rst_skinny_f32_split_plan(M, N, K) if SKINNY_F32_SPLIT is None else SKINNY_F32_SPLIT, M, N,
                        lambda: ((M + 31) // 32) * ((N + 31) // 32))
    plain = hist is None and S == 1 and P == 0 and T_in == T_out and C_ == K and act_in == ACT_NONE
    if SKINNY_F32_ROWS and plain and ln is None and not packed_in and K % 8 == 0 and x.data_ptr() % 16 == 0:
        # the rows as they are: one launch
        _lib.check(_lib.lib().rst_linear_few_rows_f32(_ptr(x), K, _ptr(wp), _ptr(bias), _ptr(res), _ptr(scale), _ptr(out), M, N, K, N, act_out,
                                                     sc[0], _ptr(sc[1]), _ptr(sc[2]), int(out_packed), _stream()))
        return
    if packed_in:
        xp = x.xp
        if not (xp.shape[1] == wp.shape[1] and ln is None and hist is None):
            raise ValueError(f"rstnet_amd.ops: a PackedRows operand of {tuple(xp.shape)} does not fit packed weights {tuple(wp.shape)} / takes no LayerNorm or history")
    else:
        xp = torch.empty(_packed_row_count(M), wp.shape[1], device=x.device, dtype=torch.float32)
        if ln is not None:
            if not plain:
                raise ValueError("rstnet_amd.ops: a LayerNorm can only be folded into the packing launch of a plain linear")
            _chk(ln[0], "ln gamma")
            _chk(ln[1], "ln beta")
            _lib.check(_lib.lib().rst_skinny_f32_pack_ln(_ptr(x), _ptr(ln[0]), _ptr(ln[1]), float(ln[2]), _ptr(xp), M, K, _stream()))
        else:
            _lib.check(_lib.lib().rst_skinny_f32_pack_win(_ptr(x), _ptr(hist), _ptr(xp), B, T_in, T_out, C_, K, S, P, pad_mode, T_in * C_, act_in,
                                                         _stream()))
    _lib.check(_lib.lib().rst_gemm_skinny_f32(_ptr(xp), _ptr(wp), _ptr(bias), _ptr(res), _ptr(scale), _ptr(out), M, N, K, N, act_out,
                                             sc[0], _ptr(sc[1]), _ptr(sc[2]), int(out_packed), _stream()))


def _few_rows(M: int, N: int, K: int) -> bool:
    # weight-bandwidth-bound shapes only: a handful of rows against at least 256 KB of weights
    return 1 <= M <= SKINNY_F32_MAX_ROWS and N * K >= 65536


def _gemm(x, hist, w, bias, res, scale, out, B, T_in, T_out, C_, K, N, S, P, pad_mode, act_in, act_out, *, ln=None,
          out_packed: bool = False, plain_linear: bool = False) -> None:
    """The one ladder of the dense fp32 GEMMs, ``out [B*T_out, N] = epi(windows(x, hist) @ w.T)``: few rows (``_gemm_few_rows``;
    ``ln`` / ``out_packed`` / a ``PackedRows`` ``x`` exist on this rung only) -> K split over workgroups -> three-plane bf16 ->
    the f32 matrix instruction (``plain_linear``: rst_linear_f32 where nothing is split)."""
    M = B * T_out
    flops = 2.0 * B * T_out * N * K
    if _few_rows(M, N, K):        # the same route with and without instrumentation: profiles describe the shipped path
        x_elems = M * K if isinstance(x, PackedRows) else x.numel()
        with _profiled("gemm_skinny_f32", flops, 4 * (w.numel() + x_elems + M * N), (M, N, K)):
            _gemm_few_rows(x, hist, w, bias, res, scale, out, B, T_in, T_out, C_, K, N, S, P, pad_mode, act_in, act_out, ln=ln,
                           out_packed=out_packed)
        return
    split_k, ws, cnt = _gemm_split_scratch(x.device, M, N, K)
    # (zero padding only: a history buffer / replicate padding keeps the launch on the f32 instruction)
    b3 = split_k <= 1 and _b3_route(x, hist, w, B, T_in, T_out, C_, K, N, S, P, pad_mode)
    nbytes = 4 * (x.numel() + w.numel() + out.numel() + (res.numel() if res is not None else 0))
    with _profiled("gemm_win_b3" if b3 else "gemm_win", flops, nbytes, (M, N, K)):
        if b3:
            _lib.check(_lib.lib().rst_gemm_win_b3_f32(_ptr(x), _ptr(hist), _ptr(w), _ptr(gemm_win_b3_pack_weight(w)), _ptr(bias), _ptr(res),
                                                      _ptr(scale), _ptr(out), B, T_in, T_out, C_, K, N, S, P, pad_mode, T_in * C_, N, act_in,
                                                      act_out, _stream()))
        elif plain_linear and split_k <= 1:
            _lib.check(_lib.lib().rst_linear_f32(_ptr(x), _ptr(w), _ptr(bias), _ptr(res), _ptr(scale), _ptr(out), M, K, N, act_out, _stream()))
        else:
            _lib.check(_lib.lib().rst_gemm_win_f32(_ptr(x), _ptr(hist), _ptr(w), _ptr(bias), _ptr(res), _ptr(scale), _ptr(out),
                                                   B, T_in, T_out, C_, K, N, S, P, pad_mode, T_in * C_, N, act_in, act_out,
                                                   split_k, _ptr(ws), _ptr(cnt), _stream()))


@_on_tensor_device
def gemm_win(x: torch.Tensor, w: torch.Tensor, *, B: int, T_in: int, T_out: int, C_: int, S: int, P: int, N: int,
             hist: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
             res: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, pad_mode: int = PAD_ZERO,
             act_in: int = ACT_NONE, act_out: int = ACT_NONE, out: Optional[torch.Tensor] = None,
             out_shape: Optional[Tuple[int, ...]] = None) -> torch.Tensor:
    """rst_gemm_win_f32.  ``w`` is ``[N, K]``; the output is ``[B*T_out, N]`` reshaped to ``out_shape``."""
    for t, n in ((x, "x"), (w, "w"), (hist, "hist"), (bias, "bias"), (res, "res"), (scale, "scale")):
        _chk(t, n)
    K = w.shape[1]
    assert w.shape[0] == N
    if out is None:
        out = torch.empty(out_shape if out_shape is not None else (B, T_out, N), device=x.device, dtype=torch.float32)
    else:
        _chk(out, "out")
    assert out.numel() == B * T_out * N, (tuple(out.shape), B, T_out, N)
    if res is not None:
        assert res.numel() == out.numel()
    if hist is not None:
        assert hist.numel() == B * P * C_, (tuple(hist.shape), B, P, C_)
    _gemm(x, hist, w, bias, res, scale, out, B, T_in, T_out, C_, K, N, S, P, pad_mode, act_in, act_out)
    return out


@_on_tensor_device
def linear(x, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, res: Optional[torch.Tensor] = None,
           scale: Optional[torch.Tensor] = None, act_out: int = ACT_NONE,
           ln: Optional[Tuple[torch.Tensor, torch.Tensor, float]] = None, out_packed: bool = False):
    """``y = epi(LN(x) @ w.T + bias)`` over the last dim of ``x`` (rst_linear_f32): the windowed GEMM with one window per row.
    ``ln = (gamma, beta, eps)``: the LayerNorm in front of the linear; it is the prologue of the launch on the one/two-position
    GEMV route, part of the packing launch on the few-row route and a separate launch otherwise.  ``out_packed`` (only where
    ``linear_chains`` says so): returns a ``PackedRows`` -- the operand of the next few-row linear in its packed order; ``x`` may be one."""
    for t, n in ((w, "w"), (bias, "bias"), (res, "res"), (scale, "scale")):
        _chk(t, n)
    packed_in = isinstance(x, PackedRows)
    if not packed_in:
        _chk(x, "x")
    N, K = w.shape[0], x.shape[-1]
    assert w.shape[1] == K
    M = math.prod(x.shape[:-1]) if K else 0
    dev = x.xp.device if packed_in else x.device
    if packed_in or out_packed:
        assert M > 4 and _few_rows(M, N, K), "packed rows travel between few-row linears only"
    if out_packed:
        assert res is None and N % 8 == 0
        out = PackedRows(torch.empty(_packed_row_count(M), N, device=dev, dtype=torch.float32), (*x.shape[:-1], N))
    else:
        out = torch.empty(*x.shape[:-1], N, device=dev, dtype=torch.float32)
    if 1 <= M <= 4 and K % 8 == 0 and K * M <= 32768 and act_out in (ACT_NONE, ACT_GELU):
        # a streaming step of one or two positions: weight-streaming GEMV (every CU pulls rows of w; no split-K hand-off)
        g, b, eps = ln if ln is not None else (None, None, 0.0)
        _chk(g, "ln gamma"); _chk(b, "ln beta")
        _lib.check(_lib.lib().rst_gemv_f32(_ptr(x), _ptr(g), _ptr(b), float(eps), _ptr(w), _ptr(bias), _ptr(res), _ptr(scale), _ptr(out),
                                           M, N, K, act_out, _stream()))
        return out
    fold_ln = ln is not None and SKINNY_F32_PACK_LN and _few_rows(M, N, K) and K % 4 == 0
    if ln is not None and not fold_ln:
        x = layernorm(x, ln[0], ln[1], ln[2])
    _gemm(x, None, w, bias, res, scale, out.xp if out_packed else out, 1, M, M, K, K, N, 1, 0, PAD_ZERO, ACT_NONE, act_out,
          ln=ln if fold_ln else None, out_packed=out_packed, plain_linear=True)
    return out


def resblock_supported(C: int, H: int, Kw: int, pre: bool = False, post: bool = False, K0: int = 0, Kf: int = 0) -> bool:
    return bool(_lib.lib().rst_seanet_resblock_supported(C, H, Kw, int(pre), int(post), K0, Kf))


@_on_tensor_device
def seanet_resblock(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, *, Kw: int,
                    hist: Optional[torch.Tensor] = None, pre: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                    post: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, elu_out: bool = False) -> torch.Tensor:
    """Fused SEANet residual block (rst_seanet_resblock_f32).  ``x [B,T,C]`` -> ``[B,T,C]``;
    ``pre=(w0 [C,K0], b0 [C])``: x is the mono audio ``[B,T,1]``; ``post=(wf [Kf,C], bf [1])``: returns ``[B,T,1]``."""
    C, H = w2.shape
    B, T = x.shape[0], x.shape[1]
    tensors = [(x, "x"), (w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (hist, "hist")]
    w0 = b0 = wf = bf = None
    K0 = Kf = 0
    if pre is not None:
        w0, b0 = pre
        K0 = w0.shape[1]
        tensors += [(w0, "w0"), (b0, "b0")]
        assert x.shape[2] == 1
    else:
        assert x.shape[2] == C
    if post is not None:
        wf, bf = post
        Kf = wf.shape[0]
        tensors += [(wf, "wf"), (bf, "bf")]
    for t, n in tensors:
        _chk(t, n)
    out = torch.empty(B, T, 1 if post is not None else C, device=x.device, dtype=torch.float32)
    # whole-utterance launches (more than 4096 rows, no streaming history): the three-plane bf16 form, as the large GEMMs
    b3 = (GEMM_B3 and hist is None and B * T > 4096 and x.data_ptr() % 16 == 0
          and _resblock_b3_supported(B, T, C, H, Kw, pre is not None, post is not None, K0, Kf))
    flops = 2.0 * B * T * (Kw * C * H + H * C) + (2.0 * B * T * C * K0) + (2.0 * B * T * C * Kf)
    with _profiled("resblock_b3" if b3 else "resblock", flops, 4 * (x.numel() + out.numel()), (B * T, C, Kw * C)):
        if b3:
            wp = resblock_b3_pack_weights(w0, w1, w2, Kw)
            _lib.check(_lib.lib().rst_seanet_resblock_b3_f32(_ptr(x), _ptr(wp), _ptr(b0), _ptr(b1), _ptr(b2), _ptr(wf), _ptr(bf), _ptr(out),
                                                             B, T, C, H, Kw, K0, Kf, int(elu_out), _stream()))
        else:
            _lib.check(_lib.lib().rst_seanet_resblock_f32(_ptr(x), _ptr(hist), _ptr(w0), _ptr(b0), _ptr(w1), _ptr(b1), _ptr(w2),
                                                          _ptr(b2), _ptr(wf), _ptr(bf), _ptr(out), B, T, C, H, Kw, K0, Kf, int(elu_out),
                                                          _stream()))
    return out


@functools.lru_cache(maxsize=256)
def _resblock_b3_supported(B: int, T: int, C: int, H: int, Kw: int, pre: bool, post: bool, K0: int, Kf: int) -> bool:
    return bool(_lib.lib().rst_seanet_resblock_b3_supported(B, T, C, H, Kw, int(pre), int(post), K0, Kf))


_rb3_weights = _PackedWeights()


@_on_tensor_device
def resblock_b3_pack_weights(w0: Optional[torch.Tensor], w1: torch.Tensor, w2: torch.Tensor, Kw: int) -> torch.Tensor:
    """The block's matrices as three bf16 planes in matrix-instruction operand order (rst_seanet_resblock_b3_pack), cached per
    storage of ``w1`` and version of all three."""
    C, H = w2.shape

    def build():
        n = int(_lib.lib().rst_seanet_resblock_b3_weight_elems(C))
        if n <= 0:
            raise ValueError(f"rstnet_amd.ops: no three-plane residual block for C = {C}")
        wp = torch.empty(n, device=w1.device, dtype=torch.int16)
        _lib.check(_lib.lib().rst_seanet_resblock_b3_pack(_ptr(w0), _ptr(w1), _ptr(w2), _ptr(wp), C, H, Kw, w0.shape[1] if w0 is not None else 0,
                                                          _stream()))
        return wp
    return _rb3_weights.get(w1, build, also=(w2, w0))


@_on_tensor_device
def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    for t, n in ((x, "x"), (gamma, "gamma"), (beta, "beta")):
        _chk(t, n)
    D = x.shape[-1]
    out = torch.empty_like(x)
    _lib.check(_lib.lib().rst_layernorm_f32(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), x.numel() // D, D, eps, _stream()))
    return out


def rope_coef(max_period: float, D: int) -> float:
    """The fp32 scalar multiplying ``arange(D/2)`` in the reference (modules/rope.py:37-38)."""
    return float(torch.tensor(-math.log(max_period) * 2 / D, dtype=torch.float32))


@_on_tensor_device
def rope_split(qkv: torch.Tensor, H: int, *, q: Optional[torch.Tensor] = None, k: Optional[torch.Tensor] = None,
               v: Optional[torch.Tensor] = None, pos0: int = 0, pos_dev: Optional[torch.Tensor] = None, ring: bool = False,
               rope: bool = True, max_period: float = 10000.0):
    """qkv ``[B,T,3*H*D]`` -> q ``[B,H,T,D]`` and k/v written into ``[B,H,cap,D]`` buffers (allocated if None)."""
    _chk(qkv, "qkv")
    B, T, E3 = qkv.shape
    D = E3 // (3 * H)
    if q is None:
        q = torch.empty(B, H, T, D, device=qkv.device, dtype=torch.float32)
    if k is None:
        assert not ring
        k = torch.empty(B, H, T, D, device=qkv.device, dtype=torch.float32)
        v = torch.empty(B, H, T, D, device=qkv.device, dtype=torch.float32)
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, n)
    if pos_dev is not None:
        _chk(pos_dev, "pos_dev", torch.int64)
        _shared_pos(pos_dev, "rope_split")
    cap = k.shape[2]
    _lib.check(_lib.lib().rst_rope_split_f32(_ptr(qkv), _ptr(q), _ptr(k), _ptr(v), _ptr(pos_dev), pos0, B, T, H, D, cap,
                                             int(ring), int(rope), rope_coef(max_period, D), _stream()))
    return q, k, v


_attn_scratch: dict = {}


@_on_tensor_device
def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, pos0: int = 0, pos_dev: Optional[torch.Tensor] = None,
              ring: bool = False, context: Optional[int] = None) -> torch.Tensor:
    """q ``[B,H,T,D]``, k/v ``[B,G,cap,D]`` (G = H, or fewer key/value heads on the few-query ring path) -> ``[B,T,H*D]``."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, n)
    B, H, T, D = q.shape
    G, cap = k.shape[1], k.shape[2]
    out = torch.empty(B, T, H * D, device=q.device, dtype=torch.float32)
    if pos_dev is not None:
        _chk(pos_dev, "pos_dev", torch.int64)
        _shared_pos(pos_dev, "attention")
    if G != H and not (ring and pos_dev is not None and D in (64, 128)):
        raise NotImplementedError("grouped key/value heads are served by the ring decode path only (head dim 64 / 128)")
    if ring and pos_dev is not None and (T <= 8 or G != H) and D in (64, 128):
        # streaming step with a handful of new queries: split every query over the occupied ring slots instead of walking
        # the ring tile by tile with one wave per head
        # (at most ~1024 workgroups: four of them fit a CU -- attn_decode_dense_kernel -- and a fifth would wait for a second round)
        splits = max(1, min(4, cap // 64, 1024 // max(1, B * T * H)))
        sc = _scratch(_attn_scratch, q.device, (B * T, H, splits, D),
                      lambda: (torch.empty(B * T, H, splits, D + 2, device=q.device, dtype=torch.float32),
                               torch.zeros(B * T, H, device=q.device, dtype=torch.int32)))
        _lib.check(_lib.lib().rst_attn_decode_multi_f32(_ptr(q), _ptr(k), _ptr(v), _ptr(sc[0]), _ptr(sc[1]), _ptr(out), _ptr(pos_dev),
                                                       B, T, H, D, cap, _ctx(context), splits, G, _stream()))
        return out
    _lib.check(_lib.lib().rst_attention_f32(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(pos_dev), pos0, B, T, H, D, cap,
                                            int(ring), _ctx(context), _stream()))
    return out


# A streaming step of a codec transformer layer's attention (a few new positions of many streams) as ONE launch: split + RoPE + ring
# append + the queries against the ring (rst_attention_step_f32).  False: rope_split + attention, two launches (the A/B switch).
ATTENTION_STEP = True
ATTENTION_STEP_PACKED = True       # its result straight in the out-projection's packed operand order on the few-row route (False: row-major)


def attention_step_serves(T: int, D: int, cap: int) -> bool:
    """Whether the library's one-launch attention step serves ``T`` new positions of head size ``D`` on a ring of ``cap`` slots -- the shape
    rule alone, asked before any tensor exists (a per-stream codec session checks it when it opens)."""
    return bool(ATTENTION_STEP and _lib.lib().rst_attention_step_supported(int(T), int(D), int(cap)))


def attention_step_supported(qkv: torch.Tensor, H: int, cap: int) -> bool:
    B, T, E3 = qkv.shape
    return bool(ATTENTION_STEP and qkv.is_cuda and E3 % (3 * H) == 0 and qkv.data_ptr() % 16 == 0 and
                _lib.lib().rst_attention_step_supported(T, E3 // (3 * H), cap))


@_on_tensor_device
def attention_step(qkv: torch.Tensor, H: int, k: torch.Tensor, v: torch.Tensor, pos_dev: torch.Tensor, *, context: Optional[int] = None,
                   rope: bool = True, max_period: float = 10000.0, out_packed: bool = False):
    """qkv ``[B,T,3*H*D]`` (the in-projection of the T new steps) -> ``[B,T,H*D]``; k / v ``[B,H,cap,D]`` rings, appended in place at
    slots ``(pos_dev + t) % cap``.  ``out_packed``: the result as a ``PackedRows`` -- the operand of the out-projection's few-row GEMM."""
    for t, n in ((qkv, "qkv"), (k, "k"), (v, "v")):
        _chk(t, n)
    _chk(pos_dev, "pos_dev", torch.int64)
    _shared_pos(pos_dev, "attention_step")
    B, T, E3 = qkv.shape
    D = E3 // (3 * H)
    if k.shape != v.shape or k.shape[0] != B or k.shape[1] != H or k.shape[3] != D:
        raise ValueError(f"rstnet_amd.ops: rings {tuple(k.shape)} / {tuple(v.shape)} do not belong to qkv {tuple(qkv.shape)} with {H} heads")
    M = B * T
    rows = _packed_row_count(M) if out_packed else 0
    if out_packed and (M > SKINNY_F32_MAX_ROWS or (H * D) % 8):
        raise ValueError(f"rstnet_amd.ops: a packed attention result needs <= {SKINNY_F32_MAX_ROWS} rows and H * D % 8 == 0 (rows {M}, H * D {H * D})")
    out = torch.empty((rows, H * D) if out_packed else (B, T, H * D), device=qkv.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_attention_step_f32(_ptr(qkv), _ptr(k), _ptr(v), _ptr(out), _ptr(pos_dev), B, T, H, D, k.shape[2],
                                                 _ctx(context), int(rope), rope_coef(max_period, D), rows, _stream()))
    return PackedRows(out, (B, T, H * D)) if out_packed else out


@_on_tensor_device
def attention_step_ps(qkv: torch.Tensor, H: int, k: torch.Tensor, v: torch.Tensor, pos_dev: torch.Tensor, *, context: Optional[int] = None,
                      rope: bool = True, max_period: float = 10000.0, out_packed: bool = False):
    """``attention_step`` with one position per stream (rst_attention_step_ps_f32): ``pos_dev`` int64 ``[B]``, stream ``b`` appends at slots
    ``(pos_dev[b] + t) % cap``, rotates by ``pos_dev[b] + t`` and sees what a stream at that position sees -- at position 0 nothing of what
    its ring held before.  Row ``b`` equals row ``b`` of ``attention_step`` launched at ``pos_dev[b]`` on the same ring, bit for bit."""
    for t, n in ((qkv, "qkv"), (k, "k"), (v, "v")):
        _chk(t, n)
    _chk(pos_dev, "pos_dev", torch.int64)
    B, T, E3 = qkv.shape
    if pos_dev.dim() != 1 or pos_dev.numel() != B:
        raise ValueError(f"rstnet_amd.ops: attention_step_ps takes one position per stream, int64 [{B}], got {tuple(pos_dev.shape)}")
    D = E3 // (3 * H)
    if k.shape != v.shape or k.shape[0] != B or k.shape[1] != H or k.shape[3] != D:
        raise ValueError(f"rstnet_amd.ops: rings {tuple(k.shape)} / {tuple(v.shape)} do not belong to qkv {tuple(qkv.shape)} with {H} heads")
    M = B * T
    rows = _packed_row_count(M) if out_packed else 0
    if out_packed and (M > SKINNY_F32_MAX_ROWS or (H * D) % 8):
        raise ValueError(f"rstnet_amd.ops: a packed attention result needs <= {SKINNY_F32_MAX_ROWS} rows and H * D % 8 == 0 (rows {M}, H * D {H * D})")
    out = torch.empty((rows, H * D) if out_packed else (B, T, H * D), device=qkv.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_attention_step_ps_f32(_ptr(qkv), _ptr(k), _ptr(v), _ptr(out), _ptr(pos_dev), 1, B, T, H, D, k.shape[2],
                                                    _ctx(context), int(rope), rope_coef(max_period, D), rows, _stream()))
    return PackedRows(out, (B, T, H * D)) if out_packed else out


_rope_tables: dict = {}
# Whole-utterance passes of the codec transformers read q / k / v in place from the in-projection's output and rotate them on load
# (rst_attention_qkv_f32).  False: rope_split + attention as two launches (the A/B switch of tools/ab.py; the streaming steps always do).
ATTENTION_FUSED_QKV = True


def rope_table(T: int, D: int, max_period: float, device) -> torch.Tensor:
    """``[T, D]`` fp32: (cos, sin) of pair i of position t at ``[t, 2i]``, ``[t, 2i + 1]`` (rst_rope_table_f32; modules/rope.py:37-62).
    ONE table per (D, max_period, device), grown to the longest pass seen (rounded up to 256 positions) and read by shorter passes as a
    prefix -- variable-length utterances launch nothing for their rotation once the longest has passed.  A table is built on the stream
    that first needs it; readers on other streams wait for the build's event, and a table replaced by a longer one stays alive with the
    tensors that reference it."""
    device = torch.device(device)
    key = (D, float(max_period), device)
    hit = _rope_tables.get(key)
    if hit is None or hit[0].shape[0] < T:
        Tp = (T + 255) // 256 * 256
        tab = torch.empty(Tp, D, device=device, dtype=torch.float32)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().rst_rope_table_f32(_ptr(tab), Tp, D, rope_coef(max_period, D), 0, _stream()))
            ev = torch.cuda.Event()
            ev.record()
            hit = _rope_tables[key] = (tab, ev, torch.cuda.current_stream())
    tab, ev, built_on = hit
    if torch.cuda.current_stream(device) != built_on and not torch.cuda.is_current_stream_capturing():
        torch.cuda.current_stream(device).wait_event(ev)
    return tab[:T]


@_on_tensor_device
def attention_qkv(qkv: torch.Tensor, H: int, *, rope: bool = True, max_period: float = 10000.0, context: Optional[int] = None) -> torch.Tensor:
    """qkv ``[B, T, 3*H*D]`` (the in-projection's output, "b t (p h d)") -> ``[B, T, H*D]``: causal (+ ``context``) attention over
    positions 0 .. T-1 with interleaved RoPE applied as q / k are loaded -- the whole-utterance pass of
    ``StreamingMultiheadAttention`` (modules/transformer.py:376-423) without the split / rotate launch and its q, k, v copies."""
    _chk(qkv, "qkv")
    B, T, E3 = qkv.shape
    D = E3 // (3 * H)
    out = torch.empty(B, T, H * D, device=qkv.device, dtype=torch.float32)
    tab = rope_table(T, D, max_period, qkv.device) if rope else None
    _lib.check(_lib.lib().rst_attention_qkv_f32(_ptr(qkv), _ptr(tab), _ptr(out), B, T, H, D, _ctx(context), _stream()))
    return out


@_on_tensor_device
def rvq_pack(emb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """emb ``[L, n_codes, D]`` -> (packed ``[L, D/8, n_codes, 2, 4]``, e2 ``[L, n_codes]``)."""
    _chk(emb, "emb")
    L, n_codes, D = emb.shape
    packed = torch.empty(L, D // 8, n_codes, 2, 4, device=emb.device, dtype=torch.float32)
    e2 = torch.empty(L, n_codes, device=emb.device, dtype=torch.float32)
    for l in range(L):
        _lib.check(_lib.lib().rst_rvq_pack_f32(_ptr(emb[l]), _ptr(packed[l]), _ptr(e2[l]), n_codes, D, _stream()))
    return packed, e2


def _int_array(vals: Sequence[int]):
    return (C.c_int * len(vals))(*vals)


def _group_arrays(groups: Sequence[Tuple[int, int]]):
    """(first level, number of levels) of every RVQ group as the two int arrays the library takes."""
    return _int_array([g[0] for g in groups]), _int_array([g[1] for g in groups])


_rvq_keys: dict = {}


# Streaming RVQ (<= 64 frames per call): all residual levels in ONE launch with in-kernel hand-offs between the code slices'
# workgroups (rst_rvq_search_chain_f32).  False: one launch per level (the A/B switch of tools/ab.py).
RVQ_CHAIN = True
_rvq_slots: dict = {}


@functools.lru_cache(maxsize=64)
def _rvq_chain_supported(dev: int, M: int, n_codes: int, L: int, D: int, n_groups: int) -> bool:
    # the library's own answer (slices x groups x frame tiles within the CUs, LDS footprint): other shapes take the per-level launches
    with torch.cuda.device(dev):
        return bool(_lib.lib().rst_rvq_chain_supported(M, n_codes, L, D, n_groups))


@_on_tensor_device
def rvq_search(x: torch.Tensor, emb: torch.Tensor, packed: torch.Tensor, e2: torch.Tensor, B: int, F: int,
               groups: Sequence[Tuple[int, int]], return_dist: bool = False):
    """x ``[B*F, n_groups*D]`` projected latents -> codes ``[B, L, F]`` int64 (levels outside ``groups`` untouched)."""
    for t, n in ((x, "x"), (emb, "emb"), (packed, "packed"), (e2, "e2")):
        _chk(t, n)
    L, n_codes, D = emb.shape
    M = B * F
    assert x.shape == (M, len(groups) * D), (tuple(x.shape), M, len(groups), D)
    covered = sorted(l for g0, n in groups for l in range(g0, g0 + n)) == list(range(L))
    codes = (torch.empty if covered else torch.zeros)(B, L, F, device=x.device, dtype=torch.int64)
    dist = torch.zeros(L, M, device=x.device, dtype=torch.float32) if return_dist else None
    keys = None
    if 0 < M <= 64 and RVQ_CHAIN and n_codes % 128 == 0 and depth_frame_enabled(x.device) and \
            _rvq_chain_supported(_device_index(x.device), M, n_codes, L, D, len(groups)):
        # streaming step, ONE launch for all levels (+ its one-workgroup finish launch): the slices' workgroups hand every level's
        # decision over in-kernel (rst_rvq_search_chain_f32); a device that had to repair falls back to the launch-per-level form below
        n_slots = int(_lib.lib().rst_rvq_chain_slot_elems(M, n_codes, L))
        sc = _scratch(_rvq_slots, x.device, (L, M, n_codes),
                      lambda: (torch.full((n_slots,), -1, device=x.device, dtype=torch.int64), new_persistent_status(x.device)))
        _lib.check(_lib.lib().rst_rvq_search_chain_f32(_ptr(x), _ptr(emb), _ptr(packed), _ptr(e2), _ptr(codes), _ptr(dist), _ptr(sc[0]), _ptr(sc[1]),
                                                       M, max(F, 1), x.shape[1], D, n_codes, L, len(groups), *_group_arrays(groups),
                                                       _stream()))
        return (codes, dist) if return_dist else codes
    if 0 < M <= 64:     # streaming step: the few-frame form (codes spread over workgroups)
        keys = _scratch(_rvq_keys, x.device, (L, M), lambda: torch.full((L, M), -1, device=x.device, dtype=torch.int64))
    _lib.check(_lib.lib().rst_rvq_search_f32(_ptr(x), _ptr(emb), _ptr(packed), _ptr(e2), _ptr(codes), _ptr(dist), _ptr(keys), M, max(F, 1),
                                             x.shape[1], D, n_codes, L, len(groups), *_group_arrays(groups), _stream()))
    return (codes, dist) if return_dist else codes


@_on_tensor_device
def rvq_gather(codes: torch.Tensor, emb: torch.Tensor, groups: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """codes ``[B, L, F]`` int64 -> ``[B*F, n_groups*D]`` sums of codebook rows per group."""
    _chk(codes, "codes", torch.int64)
    _chk(emb, "emb")
    B, L, F = codes.shape
    _, n_codes, D = emb.shape
    out = torch.empty(B * F, len(groups) * D, device=codes.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_rvq_gather_f32(_ptr(codes), _ptr(emb), _ptr(out), B * F, max(F, 1), D, n_codes, L, len(groups),
                                             *_group_arrays(groups), _stream()))
    return out


@_on_tensor_device
def convtr_depthwise(x: torch.Tensor, w: torch.Tensor, stride: int, hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x ``[B,T,C]``, w ``[C,Kw]`` -> ``[B,T*stride,C]``."""
    for t, n in ((x, "x"), (w, "w"), (hist, "hist")):
        _chk(t, n)
    B, T, Cc = x.shape
    out = torch.empty(B, T * stride, Cc, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_convtr_depthwise_f32(_ptr(x), _ptr(hist), _ptr(w), _ptr(out), B, T, Cc, w.shape[1], stride,
                                                   _stream()))
    return out


@_on_tensor_device
def activation(x: torch.Tensor, act: str) -> torch.Tensor:
    """Stand-alone ELU / GELU (only used when an activation module is called outside a fused container)."""
    _chk(x, "x")
    out = torch.empty_like(x)
    _lib.check(_lib.lib().rst_act_f32(_ptr(x), _ptr(out), x.numel(), {"elu": 1, "gelu": 2}[act], _stream()))
    return out


@_on_tensor_device
def transpose12(x: torch.Tensor) -> torch.Tensor:
    """``[B, R, C] -> [B, C, R]`` (layout adapter between the reference's [B,C,T] and channels-last)."""
    _chk(x, "x")
    B, R, Cc = x.shape
    if R == 1 or Cc == 1:
        return x.reshape(B, Cc, R)
    out = torch.empty(B, Cc, R, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_transpose_f32(_ptr(x), _ptr(out), B, R, Cc, _stream()))
    return out


@_on_tensor_device
def mask_tail(x: torch.Tensor, lengths: torch.Tensor, replicate: bool = False) -> torch.Tensor:
    """In place: rows ``t >= lengths[b]`` of ``x [B,T,C]`` become zeros (or copies of the last valid row)."""
    _chk(x, "x")
    _chk(lengths, "lengths", torch.int32)
    B, T, Cc = x.shape
    _lib.check(_lib.lib().rst_mask_tail_f32(_ptr(x), _ptr(lengths), B, T, Cc, int(replicate), _stream()))
    return x


RESAMPLE_TILE = 256     # outputs per workgroup of rst_resample_sinc (checked against the library on the first call)


def resample_staged(o: int, n: int, L: int) -> bool:
    """Whether a tile of these rates stages its inputs in LDS (False: the span is too long, the kernel reads them from global)."""
    slab = C.c_int(0)
    tile = _lib.lib().rst_resample_plan(o, n, L, C.byref(slab))
    assert tile == RESAMPLE_TILE, (tile, RESAMPLE_TILE)
    return slab.value > 0


@_on_tensor_device
def resample_sinc(x: torch.Tensor, in_lengths: Optional[torch.Tensor], filt: Optional[torch.Tensor], o: int, n: int, lead: int,
                  T_out: int, out_lengths: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Polyphase sinc rate conversion ``o : n`` of the rows of ``x [B, T_in]`` (fp32 or int16, any row stride, unit sample stride) in
    one launch -> ``y [B, T_out]`` fp32: ``y[b, i] = sum_k filt[k, i % n] * X_b[(i // n) * o + k - lead]`` for ``i < out_lengths[b]``,
    exactly 0 behind it; ``X_b`` is row ``b`` inside ``in_lengths[b]`` and zero outside (``None``: the whole row / every output).
    ``filt [L, n]`` is the TAP-MAJOR table (``audio_resample.device_table``); ``None`` at ``o == n == 1`` converts s16 -> f32 only.
    One fp32 FMA chain per output in tap order: the bits of an output do not depend on where in a batch, tile or chunk it falls
    (contract: ``rst_resample_sinc``, include/rstnet_hip.h).  Refusals raise ``RstError`` with the library's message."""
    if x.dtype not in (torch.float32, torch.int16):
        raise TypeError(f"rstnet_amd.ops: `x` must be float32 or int16, got {x.dtype}")
    _chk(x, "x", x.dtype, contiguous=False)
    _chk(in_lengths, "in_lengths", torch.int32)
    _chk(out_lengths, "out_lengths", torch.int32)
    _chk(filt, "filt")
    if x.dim() != 2 or (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        raise ValueError("rstnet_amd.ops: `x` must be [B, T_in] rows of unit sample stride")
    B, T_in = x.shape
    for t, name in ((in_lengths, "in_lengths"), (out_lengths, "out_lengths"), (filt, "filt"), (out, "out")):
        if t is not None and t.device != x.device:
            raise ValueError(f"rstnet_amd.ops: `{name}` is on {t.device}, `x` on {x.device}")
    for t, name in ((in_lengths, "in_lengths"), (out_lengths, "out_lengths")):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"rstnet_amd.ops: `{name}` must be [{B}]")
    if filt is not None and (filt.dim() != 2 or filt.shape[1] != n):
        raise ValueError(f"rstnet_amd.ops: `filt` must be the tap-major table [L, n = {n}], got {tuple(filt.shape)}")
    L = filt.shape[0] if filt is not None else 1
    T_out = int(T_out)
    if out is None:
        out = torch.empty(B, max(T_out, 0), device=x.device, dtype=torch.float32)
    else:
        _chk(out, "out", contiguous=False)
        if out.dim() != 2 or tuple(out.shape) != (B, T_out) or (T_out > 1 and out.stride(1) != 1) or (B > 1 and out.stride(0) < T_out):
            raise ValueError(f"rstnet_amd.ops: `out` must be [{B}, {T_out}] rows of unit sample stride")
    x_stride = x.stride(0) if B > 1 else T_in
    y_stride = out.stride(0) if B > 1 else max(T_out, 0)
    with _profiled("resample_sinc", 2.0 * B * max(T_out, 0) * L, x.element_size() * B * T_in + 4 * B * max(T_out, 0), (B, T_in, T_out, o, n, L)):
        rc = _lib.lib().rst_resample_sinc(_ptr(x), int(x.dtype == torch.int16), x_stride, T_in, _ptr(in_lengths), _ptr(filt), int(o), int(n), L,
                                          int(lead), _ptr(out), y_stride, _ptr(out_lengths), B, T_out, _stream())
    if rc != 0:
        raise _lib.RstError(f"librstnet_hip error {rc}: {_lib.lib().rst_last_error().decode('utf-8', 'replace')}")
    return out


def _frame_records(buf: torch.Tensor, fmt: torch.Tensor, name: str, B: int, F: int) -> int:
    _chk(buf, name, torch.uint8)
    _chk(fmt, "fmt", torch.int32)
    if buf.dim() != 2 or buf.shape[0] != B or buf.shape[1] < record_stride(F) or buf.shape[1] % 16:
        raise ValueError(f"rstnet_amd.ops: `{name}` must be uint8 [{B}, REC] with REC a multiple of 16 and >= {record_stride(F)}, "
                         f"got {tuple(buf.shape)}")
    if tuple(fmt.shape) != (B,) or fmt.device != buf.device:
        raise ValueError(f"rstnet_amd.ops: `fmt` must be int32 [{B}] on {buf.device}")
    return int(buf.shape[1])


@_on_tensor_device
def frame_ingress(staged: torch.Tensor, fmt: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Packed frame records -> the codec's input.  ``staged`` uint8 ``[B, REC]`` (per row: int32 ``present``, 12 reserved bytes, ``F``
    samples in the row's transport), ``fmt`` int32 ``[B]`` (-1 free row, 0 f32, 1 s16), ``out`` fp32 ``[B, 1, F]``: f32 bits unchanged,
    s16 as ``x / 32768``, zeros for a row without a frame or a free row (contract: ``rst_frame_ingress``, include/rstnet_hip.h)."""
    _chk(out, "out")
    if out.dim() != 3 or out.shape[1] != 1:
        raise ValueError(f"rstnet_amd.ops: `out` must be fp32 [B, 1, F], got {tuple(out.shape)}")
    B, _, F = out.shape
    rec = _frame_records(staged, fmt, "staged", B, F)
    if out.device != staged.device:
        raise ValueError(f"rstnet_amd.ops: `out` is on {out.device}, `staged` on {staged.device}")
    with _profiled("frame_ingress", 0.0, B * rec + 4 * B * F, (B, F)):
        _lib.check(_lib.lib().rst_frame_ingress(_ptr(staged), _ptr(fmt), _ptr(out), B, F, rec, _stream()))
    return out


@_on_tensor_device
def frame_egress(wav: torch.Tensor, tokens: torch.Tensor, offset_dev: torch.Tensor, max_delay: int, fmt: torch.Tensor,
                 out: torch.Tensor) -> torch.Tensor:
    """The frame's results -> packed records.  ``wav`` fp32 ``[B, 1, F]``, ``tokens`` int64 ``[B, 1 + dep_q]`` (rows of unit stride;
    the text token first), ``offset_dev`` int64 ``[B]`` (the per-stream frame counters after the commit), ``out`` uint8 ``[B, REC]``.
    A row is valid iff ``fmt[b] >= 0 and offset_dev[b] > max_delay``; header ``valid, text token or -1, payload bytes, 0``; payload f32
    as it is or s16 as ``(int16)(clamp(x, -1, 1) * 32767)``; everything else zero (contract: ``rst_frame_egress``)."""
    _chk(wav, "wav")
    _chk(tokens, "tokens", torch.int64, contiguous=False)
    _chk(offset_dev, "offset_dev", torch.int64)
    if wav.dim() != 3 or wav.shape[1] != 1:
        raise ValueError(f"rstnet_amd.ops: `wav` must be fp32 [B, 1, F], got {tuple(wav.shape)}")
    B, _, F = wav.shape
    rec = _frame_records(out, fmt, "out", B, F)
    if tokens.dim() != 2 or tokens.shape[0] != B or tokens.shape[1] < 1 or tokens.stride(1) != 1 or (B > 1 and tokens.stride(0) < 1):
        raise ValueError(f"rstnet_amd.ops: `tokens` must be int64 [{B}, n >= 1] rows of unit stride, got {tuple(tokens.shape)}")
    if tuple(offset_dev.shape) != (B,):
        raise ValueError(f"rstnet_amd.ops: `offset_dev` must be int64 [{B}] (a per-stream session), got {tuple(offset_dev.shape)}")
    for t, name in ((tokens, "tokens"), (offset_dev, "offset_dev"), (out, "out")):
        if t.device != wav.device:
            raise ValueError(f"rstnet_amd.ops: `{name}` is on {t.device}, `wav` on {wav.device}")
    tok_stride = tokens.stride(0) if B > 1 else tokens.shape[1]
    with _profiled("frame_egress", 0.0, B * rec + 4 * B * F, (B, F)):
        _lib.check(_lib.lib().rst_frame_egress(_ptr(wav), _ptr(tokens), int(tok_stride), _ptr(offset_dev), int(max_delay), _ptr(fmt),
                                               _ptr(out), B, F, rec, _stream()))
    return out


_hist_pending: Optional[list] = None      # deferred in-place rolls of the enclosing `hist_batch()` block
HIST_BATCH_MAX = 32


class hist_batch:
    """``with ops.hist_batch():`` -- the steady-state (in-place) history rolls requested inside the block are deferred and run as
    ONE launch at its end (rst_hist_update_batch_f32).  Valid because a layer's history is read only by that layer's own
    convolution, which has run by then; the block keeps the layer inputs alive until the roll."""

    def __enter__(self):
        global _hist_pending
        self._outer = _hist_pending
        _hist_pending = []
        return self

    def __exit__(self, *exc):
        global _hist_pending
        pending, _hist_pending = _hist_pending, self._outer
        if exc[0] is None:
            flush_hist_updates(pending)
        return False


def flush_hist_updates(pending: list) -> None:
    for i in range(0, len(pending), HIST_BATCH_MAX):
        part = pending[i:i + HIST_BATCH_MAX]
        n, B = len(part), part[0][0].shape[0]
        xs = (C.c_void_p * n)(*[x.data_ptr() for x, _ in part])
        hs = (C.c_void_p * n)(*[h.data_ptr() for _, h in part])
        ti, pp, cc = _int_array([x.shape[1] for x, _ in part]), _int_array([h.shape[1] for _, h in part]), _int_array([h.shape[2] for _, h in part])
        with torch.cuda.device(part[0][0].device):
            _lib.check(_lib.lib().rst_hist_update_batch_f32(xs, hs, ti, pp, cc, n, B, _stream()))


@_on_tensor_device
def hist_update(x: torch.Tensor, hist_in: Optional[torch.Tensor], P_out: int) -> torch.Tensor:
    """Last ``P_out`` steps of concat(hist_in, x) along time; x ``[B,T,C]``, hist ``[B,P,C]``.  In steady state (same history
    length, at most 16384 elements per stream) the roll happens IN PLACE and ``hist_in`` itself is returned: the state keeps
    its address, which is what lets a whole codec step be replayed as a HIP graph."""
    _chk(x, "x")
    _chk(hist_in, "hist_in")
    B, T, Cc = x.shape
    P_in = hist_in.shape[1] if hist_in is not None else 0
    if hist_in is not None and P_in == P_out and P_out * Cc <= 16384 and P_out > 0:
        if _hist_pending is not None and (not _hist_pending or _hist_pending[0][0].shape[0] == B):
            _hist_pending.append((x, hist_in))       # rolled by the enclosing hist_batch() block, in one launch with its peers
            return hist_in
        _lib.check(_lib.lib().rst_hist_update_f32(_ptr(x), _ptr(hist_in), _ptr(hist_in), B, T, P_in, P_out, Cc, _stream()))
        return hist_in
    out = torch.empty(B, P_out, Cc, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_hist_update_f32(_ptr(x), _ptr(hist_in), _ptr(out), B, T, P_in, P_out, Cc, _stream()))
    return out


@_on_tensor_device
def hist_seed(x: Optional[torch.Tensor], hist: torch.Tensor, fresh: torch.Tensor, *, replicate: bool) -> None:
    """Streams that start over inside a live batch (rst_hist_seed_f32): where ``fresh[b]`` (int32 ``[B]`` on the device) is set, the
    history row ``hist[b]`` ``[P, C]`` becomes what a new session's first chunk finds -- ``P`` copies of ``x[b, 0]`` (``replicate``; ``x``
    ``[B, T, C]`` is that chunk) or zeros -- and the flag is cleared; the other rows keep their bytes.  In place, one launch."""
    _chk(x, "x")
    _chk(hist, "hist")
    _chk(fresh, "fresh", torch.int32)
    B, P, Cc = hist.shape
    if fresh.numel() != B or (x is not None and (x.dim() != 3 or x.shape[0] != B or x.shape[2] != Cc)):
        raise ValueError(f"rstnet_amd.ops: hist_seed: history {tuple(hist.shape)} against flags {tuple(fresh.shape)} / chunk "
                         f"{None if x is None else tuple(x.shape)}")
    if replicate and (x is None or x.shape[1] < 1):
        raise ValueError("rstnet_amd.ops: hist_seed: replicate padding needs the chunk's first step")
    _lib.check(_lib.lib().rst_hist_seed_f32(_ptr(x), _ptr(hist), _ptr(fresh), B, 0 if x is None else x.shape[1], P, Cc, int(replicate), _stream()))


# ----------------------------------------------------------------------------------------------------------------------
# RQ-Transformer decode step (T = 1, small batch): bf16 weights, fp32 activations
# ----------------------------------------------------------------------------------------------------------------------
PROLOGUE_NONE, PROLOGUE_RMSNORM, PROLOGUE_SILU_GATE = 0, 1, 2


@_on_tensor_device
def gemv_bf16(x: torch.Tensor, w: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
              eps: float = 1e-8, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, gate_out: bool = False) -> torch.Tensor:
    """``y[B,N] = (res +) (bias +) P(x) @ w.T`` with ``w`` bf16 ``[N,K]`` (rst_gemv_bf16_f32).  ``x`` is fp32 ``[B,K]``
    (``[B,2K]`` for the SiLU-gate prologue).  ``gate_out`` (``w = [W_u ; W_v]``): returns ``silu(u) * v`` of shape ``[B, N/2]``."""
    _chk(x, "x")
    _chk(w, "w", torch.bfloat16)
    _chk(alpha, "alpha")
    _chk(res, "res")
    _chk(bias, "bias")
    B = x.shape[0]
    N, K = w.shape
    assert x.shape[1] == (2 * K if prologue == PROLOGUE_SILU_GATE else K), (tuple(x.shape), N, K, prologue)
    No = N // 2 if gate_out else N
    if out is None:
        out = torch.empty(B, No, device=x.device, dtype=torch.float32)
    with _profiled("gemv_bf16", 2.0 * B * N * K, 2 * N * K + 4 * (x.numel() + out.numel()), (B, N, K)):
        _lib.check(_lib.lib().rst_gemv_bf16_f32(_ptr(x), _ptr(alpha), _ptr(w), _ptr(res), _ptr(bias), _ptr(out), B, N, K, x.shape[1], No,
                                               prologue, eps, int(gate_out), _stream()))
    return out


@_on_tensor_device
def quantize_rows_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[N, K]`` -> (``q`` uint8 ``[N, K]``: OCP e4m3fn bytes, ``scale`` fp32 ``[N]``: one power of two per row, the smallest
    with ``amax / scale <= 448``; rst_quant_rows_fp8).  ``q * scale`` is exactly a bf16 number.  Non-finite weights raise."""
    _chk(w, "w", torch.bfloat16)
    assert w.dim() == 2, tuple(w.shape)
    if not bool(torch.isfinite(w).all()):
        raise ValueError("rstnet_amd.ops.quantize_rows_fp8: the weight holds non-finite values")
    N, K = w.shape
    q = torch.empty(N, K, device=w.device, dtype=torch.uint8)
    scale = torch.empty(N, device=w.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_quant_rows_fp8(_ptr(w), _ptr(q), _ptr(scale), N, K, _stream()))
    return q, scale


def dequantize_rows_fp8(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The bf16 ``[N, K]`` matrix that ``(q, scale)`` of ``quantize_rows_fp8`` stands for (exact: 4 significant bits times a power of two)."""
    return (q.view(torch.float8_e4m3fn).to(torch.float32) * scale[:, None]).to(torch.bfloat16)


def gemv_fp8w_supported(B: int, N: int, K: int) -> bool:
    """Shapes ``gemv_fp8w`` serves (``K % 16 == 0``, ``B <= 4``, ``B * roundup(K, 1024) <= 32768``); others take the bf16 weight."""
    return bool(_lib.lib().rst_gemv_fp8w_supported(B, N, K))


def _gemv_quant(op: str, x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, K: int, scale_dtype, scale_shape: tuple, wbytes: int,
                prologue: int, alpha, eps: float, res, bias, out, gate_out: bool) -> torch.Tensor:
    """The body of ``gemv_fp8w`` and ``gemv_mxfp4w``: argument checks, output, the profile row ``op`` and the launch ``rst_<op>_f32``.
    ``K``, the scales' dtype and shape and ``wbytes`` (weight + scale bytes streamed) are what the two formats differ in."""
    _chk(x, "x")
    _chk(q, "q", torch.uint8)
    _chk(scale, "scale", scale_dtype)
    _chk(alpha, "alpha")
    _chk(res, "res")
    _chk(bias, "bias")
    B, N = x.shape[0], q.shape[0]
    assert scale.shape == scale_shape, (tuple(q.shape), tuple(scale.shape))
    assert x.shape[1] == (2 * K if prologue == PROLOGUE_SILU_GATE else K), (tuple(x.shape), N, K, prologue)
    No = N // 2 if gate_out else N
    if out is None:
        out = torch.empty(B, No, device=x.device, dtype=torch.float32)
    with _profiled(op, 2.0 * B * N * K, wbytes + 4 * (x.numel() + out.numel()), (B, N, K)):
        _lib.check(getattr(_lib.lib(), f"rst_{op}_f32")(_ptr(x), _ptr(alpha), _ptr(q), _ptr(scale), _ptr(res), _ptr(bias), _ptr(out), B, N, K,
                                                       x.shape[1], No, prologue, eps, int(gate_out), _stream()))
    return out


@_on_tensor_device
def gemv_fp8w(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
              eps: float = 1e-8, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, gate_out: bool = False) -> torch.Tensor:
    """``gemv_bf16`` on fp8 weight storage: ``y[B,N] = (res +) (bias +) scale * (P(x) @ q.T)`` with ``q`` e4m3fn bytes ``[N,K]`` and
    one fp32 scale per row (``quantize_rows_fp8``; rst_gemv_fp8w_f32).  The scale multiplies the dot product only."""
    N, K = q.shape
    return _gemv_quant("gemv_fp8w", x, q, scale, K, torch.float32, (N,), N * K + 4 * N, prologue, alpha, eps, res, bias, out, gate_out)


_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


class Mxfp4Copy(NamedTuple):
    """``(q, scale)`` of ``quantize_blocks_mxfp4``, typed so that ``lm_linear`` / ``lm_gated_pair`` can tell it from an fp8 ``(q, scale)``
    pair in their ``w8=`` / ``w8_in=`` / ``w8_out=`` arguments."""
    q: torch.Tensor
    scale: torch.Tensor


class Mxfp4BatchedCopy(Mxfp4Copy):
    """An ``Mxfp4Copy`` whose owner opted in to the batched route (``LMModel.quantize_weights_("mxfp4", batched=True)``): the same two
    fields, and ``lm_linear`` / ``lm_gated_pair`` stream it above two rows too (``gemm_skinny_mxfp4w``) instead of reading the bf16
    weight there."""
    __slots__ = ()


@_on_tensor_device
def quantize_blocks_mxfp4(w: torch.Tensor) -> "Mxfp4Copy":
    """bf16 ``[N, K]``, ``K % 32 == 0`` -> (``q`` uint8 ``[N, K/2]``: OCP e2m1 codes, two per byte, even ``k`` in the low nibble;
    ``scale`` uint8 ``[N, K/32]``: ``e + 127`` per block of 32 ``k``, ``e`` the smallest integer with ``amax / 2^e <= 6``, at least
    -125; rst_quant_blocks_mxfp4).  ``code * 2^e`` is exactly a bf16 number.  Non-finite weights and ``|w| >= 2^120`` raise."""
    _chk(w, "w", torch.bfloat16)
    assert w.dim() == 2, tuple(w.shape)
    N, K = w.shape
    if K % 32:
        raise ValueError(f"rstnet_amd.ops.quantize_blocks_mxfp4: K = {K} is not a multiple of the block size 32")
    if not bool(torch.isfinite(w).all()) or bool((w.abs() >= 2.0 ** 120).any()):
        raise ValueError("rstnet_amd.ops.quantize_blocks_mxfp4: the weight holds non-finite values or magnitudes >= 2^120")
    q = torch.empty(N, K // 2, device=w.device, dtype=torch.uint8)
    scale = torch.empty(N, K // 32, device=w.device, dtype=torch.uint8)
    _lib.check(_lib.lib().rst_quant_blocks_mxfp4(_ptr(w), _ptr(q), _ptr(scale), N, K, _stream()))
    return Mxfp4Copy(q, scale)


def dequantize_blocks_mxfp4(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The bf16 ``[N, K]`` matrix that ``(q, scale)`` of ``quantize_blocks_mxfp4`` stands for (exact: 2 significant bits times a
    power of two, a normal number)."""
    N = q.shape[0]
    codes = torch.stack((q & 0xF, q >> 4), dim=-1).view(N, -1).long()
    mag = torch.tensor(_E2M1_VALUES, device=q.device, dtype=torch.float32)[codes & 7]
    val = torch.where(codes >= 8, -mag, mag).view(N, -1, 32) * torch.exp2(scale.to(torch.float32) - 127.0)[:, :, None]
    return val.view(N, -1).to(torch.bfloat16)


def gemv_mxfp4w_supported(B: int, N: int, K: int) -> bool:
    """Shapes ``gemv_mxfp4w`` serves (``K % 32 == 0``, ``B <= 4``, ``B * roundup(K, 2048) <= 32768``); others take fp8 or bf16."""
    return bool(_lib.lib().rst_gemv_mxfp4w_supported(B, N, K))


@_on_tensor_device
def gemv_mxfp4w(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
                eps: float = 1e-8, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, gate_out: bool = False) -> torch.Tensor:
    """``gemv_bf16`` on MXFP4 weight storage: ``y[B,N] = (res +) (bias +) P(x) @ dequantize_blocks_mxfp4(q, scale).T`` with ``q`` packed
    e2m1 codes ``[N,K/2]`` and one scale byte per 32 ``k`` (``quantize_blocks_mxfp4``; rst_gemv_mxfp4w_f32)."""
    N, K = q.shape[0], 2 * q.shape[1]
    assert K % 32 == 0, tuple(q.shape)
    return _gemv_quant("gemv_mxfp4w", x, q, scale, K, torch.uint8, (N, K // 32), N * K // 2 + N * K // 32, prologue, alpha, eps, res, bias, out,
                       gate_out)


# Measured on MI355X (tools/bench_depth.py, graph-replayed chains at the depth transformer's shape): the out-projection with the
# attention as its prologue costs 8.8 us per launch against 4.0 us (plain out-projection) + 3.2 us (attn_small) for the two
# launches it replaces -- the prologue's dependent chain (qkv row -> 16 K/V rows -> scores -> softmax -> LDS) is longer than a
# kernel boundary.  The fused form stays available (and tested) but is not the default.
FUSE_SHORT_RING_ATTENTION = False


def gemv_attn_supported(B: int, H: int, D: int, cap: int, rope: bool, G: Optional[int] = None) -> bool:
    """Whether ``gemv_attn`` serves this attention AND is wanted: batch <= 2, a ring of <= 8 slots, no rotary embedding, one kv
    head per query head and a power-of-two head dim -- the depth transformer of both LM families."""
    return FUSE_SHORT_RING_ATTENTION and B <= 2 and 1 <= cap <= 8 and not rope and (G is None or G == H) and 4 <= D <= 256 and D & (D - 1) == 0 and B * H * D <= 32768


@_on_tensor_device
def gemv_attn(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos_dev: torch.Tensor, w: torch.Tensor, *,
              context: Optional[int] = None, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``res + W_out attention(qkv)`` in ONE launch (rst_gemv_attn_bf16_f32): ``qkv [B, 3*H*D]`` un-rotated, the ring
    ``[B, H, cap <= 8, D]`` (the new step is appended by the launch), ``w`` bf16 ``[N, H*D]``."""
    _chk(qkv, "qkv"); _chk(k_cache, "k_cache"); _chk(v_cache, "v_cache"); _chk(res, "res"); _chk(bias, "bias")
    _chk(pos_dev, "pos_dev", torch.int64)
    _shared_pos(pos_dev, "gemv_attn")
    _chk(w, "w", torch.bfloat16)
    B, H, cap, D = k_cache.shape
    N = w.shape[0]
    assert qkv.shape == (B, 3 * H * D) and w.shape[1] == H * D, (tuple(qkv.shape), tuple(w.shape), H, D)
    out = torch.empty(B, N, device=qkv.device, dtype=torch.float32)
    with _profiled("gemv_bf16", 2.0 * B * N * H * D, 2 * N * H * D + 4 * (qkv.numel() + out.numel()), (B, N, H * D)):
        _lib.check(_lib.lib().rst_gemv_attn_bf16_f32(_ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(pos_dev), _ptr(w), _ptr(res), _ptr(bias),
                                                    _ptr(out), B, N, H, D, cap, _ctx(context), qkv.shape[1], N, _stream()))
    return out


@_on_tensor_device
def gemv_embed(add: torch.Tensor, table: torch.Tensor, tokens: torch.Tensor, col: int, w: torch.Tensor, *, alpha: torch.Tensor,
               eps: float = 1e-8, bias: Optional[torch.Tensor] = None):
    """First GEMV of a depth step (rst_gemv_embed_bf16_f32): ``x = add + table[tokens[:, col]]`` (``add`` fp32 ``[B, K]``, possibly a
    column block of a wider row-major buffer: unit column stride, any row stride), ``y = RMSNorm(x) @ w.T``.  Returns ``(y, x)``."""
    _chk(tokens, "tokens", torch.int64)
    _chk(table, "table", torch.bfloat16)
    _chk(w, "w", torch.bfloat16)
    _chk(alpha, "alpha"); _chk(bias, "bias")
    if not add.is_cuda or add.dtype != torch.float32 or add.dim() != 2 or add.stride(1) != 1:
        raise ValueError("rstnet_amd.ops: `add` must be a float32 CUDA/HIP matrix with unit column stride")
    B, K = add.shape
    N = w.shape[0]
    assert w.shape[1] == K and table.shape[1] == K and tokens.shape[0] == B and 0 <= col < tokens.shape[1]
    y = torch.empty(B, N, device=add.device, dtype=torch.float32)
    x = torch.empty(B, K, device=add.device, dtype=torch.float32)
    with _profiled("gemv_bf16", 2.0 * B * N * K, 2 * N * K + 4 * (2 * B * K + y.numel()), (B, N, K)):
        _lib.check(_lib.lib().rst_gemv_embed_bf16_f32(_ptr(add), _ptr(table), _ptr(tokens), _ptr(x), _ptr(alpha), _ptr(w), _ptr(bias), _ptr(y),
                                                     B, N, K, add.stride(0) if B > 1 else K, N, tokens.shape[1], col, table.shape[0], float(eps),
                                                     _stream()))
    return y, x


_skinny_weights = _PackedWeights()
_skinny_weights_gated = _PackedWeights()


@_on_tensor_device
def skinny_pack_weight(w: torch.Tensor, interleave_halves: bool = False) -> torch.Tensor:
    """bf16 ``[N, K]`` -> the MFMA-ordered copy ``[ceil(N/32)*32, K]`` of rst_skinny_pack_weight_bf16, cached per weight
    storage (the row-major original stays: the batch <= 2 GEMV streams that one).  ``interleave_halves``: the layout of gated
    layers (``w = [W_u ; W_v]``) whose GEMM applies ``silu(u) * v`` in its epilogue."""
    _chk(w, "w", torch.bfloat16)
    N, K = w.shape

    def build():
        wp = torch.empty((N + 31) // 32 * 32, K, device=w.device, dtype=torch.bfloat16)
        _lib.check(_lib.lib().rst_skinny_pack_weight_bf16(_ptr(w), _ptr(wp), N, K, int(interleave_halves), _stream()))
        return wp
    return (_skinny_weights_gated if interleave_halves else _skinny_weights).get(w, build)


@_on_tensor_device
def skinny_pack_act(x: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
                    eps: float = 1e-8) -> torch.Tensor:
    """fp32 ``[B, K]`` (``[B, 2K]`` for the SiLU gate) -> packed bf16 hi / lo planes ``[2, ceil(B/32)*32, K]`` of P(x)."""
    _chk(x, "x")
    _chk(alpha, "alpha")
    B = x.shape[0]
    K = x.shape[1] // 2 if prologue == PROLOGUE_SILU_GATE else x.shape[1]
    xp = torch.empty(2, (B + 31) // 32 * 32, K, device=x.device, dtype=torch.bfloat16)
    _lib.check(_lib.lib().rst_skinny_pack_act_f32(_ptr(x), _ptr(alpha), _ptr(xp), B, K, x.shape[1], prologue, eps, _stream()))
    return xp


class PackedAct(NamedTuple):
    """Activations already in the skinny GEMM's operand form (bf16 hi / lo planes ``[2, ceil(B/32)*32, K]``, rows past B zero),
    as emitted directly by a producer kernel (``lm_attn_decode(..., packed=True)``)."""
    xp: torch.Tensor
    B: int
    K: int


_packed_out: dict = {}


def _packed_buffer(device, B: int, K: int, role: str = "in") -> torch.Tensor:
    """Persistent, zero-initialised operand buffer per (stream, shape): producers write rows < B only, so the pad rows stay zero;
    layers of equal shape share it (launches on one stream are ordered).  ``role`` keeps the output of a GEMM that emits a packed
    operand apart from the operand it reads."""
    return _scratch(_packed_out, device, (B, K, role), lambda: torch.zeros(2, (B + 31) // 32 * 32, K, device=device, dtype=torch.bfloat16))


# K up to which a plain / RMSNorm linear of 2 < B <= 64 rows takes the fp32 activations directly (rst_gemm_skinny_x32_bf16_f32: the
# operand is formed inside the GEMM, no packing launch); above it the packing launch + packed GEMM (+ K split) stay
SKINNY_X32_MAX_K = 2048


def _gemm_skinny_packed(op: str, entry: str, x, wptrs: tuple, wbytes: int, N: int, K: int, prologue: int, alpha, eps: float, res, bias,
                        gate_out: bool):
    """The body of ``gemm_skinny`` (past its fp32-input form), ``gemm_skinny_fp8w`` and ``gemm_skinny_mxfp4w``: the packed activations
    (a ``PackedAct`` as is, fp32 rows through ``skinny_pack_act``), the output, the profile row ``op`` and the launch ``entry`` on the
    bf16 route's split plan.  ``wptrs`` (the packed weight and what goes with it) and ``wbytes`` (weight + scale bytes streamed) are
    what the formats differ in."""
    if isinstance(x, PackedAct):
        assert prologue == PROLOGUE_NONE and x.K == K
        xp, B = x.xp, x.B
        x = xp
    else:
        B = x.shape[0]
        xp = skinny_pack_act(x, prologue=prologue, alpha=alpha, eps=eps)
    assert xp.shape[2] == K, (tuple(x.shape), N, K, prologue)
    # gate_out: the weight is a stacked [W_u ; W_v]; the epilogue emits silu(u) * v as the packed operand of the next GEMM
    out = None if gate_out else torch.empty(B, N, device=x.device, dtype=torch.float32)
    gp = _packed_buffer(x.device, B, N // 2, "gate") if gate_out else None
    with _profiled(op, 2.0 * B * N * K, wbytes + 4 * (x.numel() + B * N), (B, N, K)):
        # one launch plan and scratch for every weight format (same shape key: launches on one stream are ordered)
        sc = _split_scratch(xp.device, ("skinny_bf16", B, N, K), lambda: _lib.lib().rst_skinny_bf16_split_plan(B, N, K),
                            (B + 31) // 32 * 32, N, lambda: (N + 31) // 32)
        _lib.check(getattr(_lib.lib(), entry)(_ptr(xp), *wptrs, _ptr(res), _ptr(bias), _ptr(out), B, N, K, N, _ptr(gp),
                                              sc[0], _ptr(sc[1]), _ptr(sc[2]), _stream()))
    return PackedAct(gp, B, N // 2) if gate_out else out


@_on_tensor_device
def gemm_skinny(x, w: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
                eps: float = 1e-8, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, gate_out: bool = False):
    """``y[B,N] = (res +) (bias +) P(x) @ w.T`` for 2 < B <= 64 on the bf16 matrix cores: prologue + hi/lo split + packing of
    the activations (one small launch; skipped when ``x`` is a ``PackedAct``), then rst_gemm_skinny_bf16_f32 against the packed
    copy of ``w``."""
    _chk(res, "res")
    _chk(bias, "bias")
    N, K = w.shape
    gate_out = gate_out and N % 32 == 0 and res is None
    wp = skinny_pack_weight(w, interleave_halves=gate_out)
    if not isinstance(x, PackedAct) and prologue in (PROLOGUE_NONE, PROLOGUE_RMSNORM) and K <= SKINNY_X32_MAX_K and K % 256 == 0 and x.dim() == 2 and \
            x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0:      # (K this short is never split: split plan >= 4096)
        # fp32 rows straight into the GEMM (one launch instead of two)
        _chk(alpha, "alpha")
        if not x.is_cuda or x.dtype != torch.float32:
            raise TypeError("rstnet_amd.ops: `x` must be a float32 CUDA/HIP matrix")
        assert x.shape[1] == K, (tuple(x.shape), N, K, prologue)
        B = x.shape[0]
        out = None if gate_out else torch.empty(B, N, device=x.device, dtype=torch.float32)
        gp = _packed_buffer(x.device, B, N // 2, "gate") if gate_out else None
        with _profiled("gemm_skinny", 2.0 * B * N * K, 2 * N * K + 4 * (x.numel() + B * N), (B, N, K)):
            _lib.check(_lib.lib().rst_gemm_skinny_x32_bf16_f32(_ptr(x), _ptr(alpha) if prologue == PROLOGUE_RMSNORM else None, float(eps),
                                                              1 if prologue == PROLOGUE_RMSNORM else 0, x.stride(0) if B > 1 else K, _ptr(wp),
                                                              _ptr(res), _ptr(bias), _ptr(out), B, N, K, N, _ptr(gp), _stream()))
        return PackedAct(gp, B, N // 2) if gate_out else out
    return _gemm_skinny_packed("gemm_skinny", "rst_gemm_skinny_bf16_f32", x, (_ptr(wp),), 2 * N * K, N, K, prologue, alpha, eps, res, bias, gate_out)


_skinny_weights_fp8w = _PackedWeights()
_skinny_weights_fp8w_gated = _PackedWeights()


def gemm_skinny_fp8w_supported(B: int, N: int, K: int) -> bool:
    """Shapes ``gemm_skinny_fp8w`` serves (``1 <= B <= 64``, ``K % 32 == 0``, any ``N``); others take the bf16 weight."""
    return bool(_lib.lib().rst_gemm_skinny_fp8w_supported(B, N, K))


@_on_tensor_device
def skinny_pack_weight_fp8w(q: torch.Tensor, scale: torch.Tensor, interleave_halves: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(q, scale)`` of ``quantize_rows_fp8`` -> (``qp`` uint8 ``[ceil(N/32)*32, K]``: the bytes in the MFMA order of
    rst_skinny_pack_weight_fp8w, pad rows zero; ``sp`` fp32 ``[ceil(N/32)*32]``: the scales in the same row order, pad rows 0), cached
    per ``q`` storage (the row-major ``q`` stays: the batch <= 2 GEMV streams that one).  ``interleave_halves``: the layout of gated
    layers, as ``skinny_pack_weight``."""
    _chk(q, "q", torch.uint8)
    _chk(scale, "scale")
    N, K = q.shape
    assert scale.shape == (N,), (tuple(q.shape), tuple(scale.shape))
    if K % 32:
        raise ValueError(f"rstnet_amd.ops.skinny_pack_weight_fp8w: K = {K} is not a multiple of 32")

    def build():
        n32 = (N + 31) // 32 * 32
        qp = torch.empty(n32, K, device=q.device, dtype=torch.uint8)
        sp = torch.empty(n32, device=q.device, dtype=torch.float32)
        _lib.check(_lib.lib().rst_skinny_pack_weight_fp8w(_ptr(q), _ptr(scale), _ptr(qp), _ptr(sp), N, K, int(interleave_halves), _stream()))
        return qp, sp
    return (_skinny_weights_fp8w_gated if interleave_halves else _skinny_weights_fp8w).get(q, build, also=(scale,))


@_on_tensor_device
def gemm_skinny_fp8w(x, q: torch.Tensor, scale: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
                     eps: float = 1e-8, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, gate_out: bool = False):
    """``gemm_skinny`` on fp8 weight storage: ``y[B,N] = (res +) (bias +) scale * (P(x) @ q.T)`` for 1 <= B <= 64, ``q`` e4m3fn bytes
    ``[N,K]`` with one power-of-two fp32 scale per row (``quantize_rows_fp8``).  ``x``: fp32 rows (packed into bf16 hi / lo planes by one
    small launch, with the prologue) or a ``PackedAct``; the weight bytes are decoded to bf16 inside rst_gemm_skinny_fp8w_f32 (exact) and
    the scale multiplies the fp32 accumulators: the values of ``gemm_skinny`` on ``dequantize_rows_fp8(q, scale)`` from half the
    weight bytes.  ``gate_out``: as ``gemm_skinny`` (returns a ``PackedAct``)."""
    _chk(res, "res")
    _chk(bias, "bias")
    N, K = q.shape
    B = x.B if isinstance(x, PackedAct) else x.shape[0]
    if not gemm_skinny_fp8w_supported(B, N, K):
        raise ValueError(f"rstnet_amd.ops.gemm_skinny_fp8w: no fp8 weight-only skinny GEMM for B = {B}, N = {N}, K = {K} "
                         "(1 <= B <= 64 and K % 32 == 0 required)")
    gate_out = gate_out and N % 32 == 0 and res is None
    qp, sp = skinny_pack_weight_fp8w(q, scale, interleave_halves=gate_out)
    return _gemm_skinny_packed("gemm_skinny_fp8w", "rst_gemm_skinny_fp8w_f32", x, (_ptr(qp), _ptr(sp)), N * K + 4 * N, N, K, prologue, alpha, eps,
                               res, bias, gate_out)


_skinny_weights_mxfp4w = _PackedWeights()
_skinny_weights_mxfp4w_gated = _PackedWeights()


def gemm_skinny_mxfp4w_supported(B: int, N: int, K: int) -> bool:
    """Shapes ``gemm_skinny_mxfp4w`` serves (``1 <= B <= 64``, ``K % 32 == 0``, any ``N``); others take the bf16 weight."""
    return bool(_lib.lib().rst_gemm_skinny_mxfp4w_supported(B, N, K))


@_on_tensor_device
def skinny_pack_weight_mxfp4w(q: torch.Tensor, scale: torch.Tensor, interleave_halves: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(q, scale)`` of ``quantize_blocks_mxfp4`` -> (``qp`` uint8 ``[ceil(N/32)*32, K/2]``: the code bytes in the MFMA order of
    rst_skinny_pack_weight_mxfp4w, pad rows zero; ``sp`` uint8 ``[ceil(N/32), K/32, 32]``: the scale bytes per tile, block and row, pad
    rows 127), cached per ``q`` storage (the row-major ``q`` stays: the batch <= 2 GEMV streams that one).  One copy serves every
    batch size.  ``interleave_halves``: the layout of gated layers, as ``skinny_pack_weight``."""
    _chk(q, "q", torch.uint8)
    _chk(scale, "scale", torch.uint8)
    N, K = q.shape[0], 2 * q.shape[1]
    if K % 32:
        raise ValueError(f"rstnet_amd.ops.skinny_pack_weight_mxfp4w: K = {K} is not a multiple of 32")
    assert scale.shape == (N, K // 32), (tuple(q.shape), tuple(scale.shape))

    def build():
        t32 = (N + 31) // 32
        qp = torch.empty(t32 * 32, K // 2, device=q.device, dtype=torch.uint8)
        sp = torch.empty(t32, K // 32, 32, device=q.device, dtype=torch.uint8)
        _lib.check(_lib.lib().rst_skinny_pack_weight_mxfp4w(_ptr(q), _ptr(scale), _ptr(qp), _ptr(sp), N, K, int(interleave_halves), _stream()))
        return qp, sp
    return (_skinny_weights_mxfp4w_gated if interleave_halves else _skinny_weights_mxfp4w).get(q, build, also=(scale,))


@_on_tensor_device
def gemm_skinny_mxfp4w(x, q: torch.Tensor, scale: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
                       eps: float = 1e-8, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, gate_out: bool = False):
    """``gemm_skinny`` on MXFP4 weight storage: ``y[B,N] = (res +) (bias +) P(x) @ dequantize_blocks_mxfp4(q, scale).T`` for
    1 <= B <= 64, ``q`` packed e2m1 codes ``[N,K/2]`` with one scale byte per 32 ``k`` (``quantize_blocks_mxfp4``).  ``x``: fp32 rows
    (packed into bf16 hi / lo planes by one small launch, with the prologue) or a ``PackedAct``; the codes are decoded times their block
    scale to the bf16 operand inside rst_gemm_skinny_mxfp4w_f32 (exact), so the values are those of ``gemm_skinny`` on the dequantised
    matrix, bit for bit, from a quarter of the weight bytes.  ``gate_out``: as ``gemm_skinny`` (returns a ``PackedAct``)."""
    _chk(res, "res")
    _chk(bias, "bias")
    N, K = q.shape[0], 2 * q.shape[1]
    B = x.B if isinstance(x, PackedAct) else x.shape[0]
    if not gemm_skinny_mxfp4w_supported(B, N, K):
        raise ValueError(f"rstnet_amd.ops.gemm_skinny_mxfp4w: no MXFP4 weight-only skinny GEMM for B = {B}, N = {N}, K = {K} "
                         "(1 <= B <= 64 and K % 32 == 0 required)")
    gate_out = gate_out and N % 32 == 0 and res is None
    qp, sp = skinny_pack_weight_mxfp4w(q, scale, interleave_halves=gate_out)
    return _gemm_skinny_packed("gemm_skinny_mxfp4w", "rst_gemm_skinny_mxfp4w_f32", x, (_ptr(qp), _ptr(sp)), N * K // 2 + N * K // 32, N, K,
                               prologue, alpha, eps, res, bias, gate_out)


_skinny_weights_fp8 = _PackedWeights()


@_on_tensor_device
def skinny_pack_weight_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[N, K]`` -> (fp8 e4m3 copy in MFMA order ``[ceil(N/32)*32, K]`` uint8, per-row scales fp32), cached per weight."""
    _chk(w, "w", torch.bfloat16)
    N, K = w.shape

    def build():
        n32 = (N + 31) // 32 * 32
        wp = torch.empty(n32, K, device=w.device, dtype=torch.uint8)
        sc = torch.empty(n32, device=w.device, dtype=torch.float32)
        _lib.check(_lib.lib().rst_skinny_pack_weight_fp8(_ptr(w), _ptr(wp), _ptr(sc), N, K, _stream()))
        return wp, sc
    return _skinny_weights_fp8.get(w, build)


@_on_tensor_device
def gemm_skinny_fp8(x: torch.Tensor, w: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
                    eps: float = 1e-8, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The fp8 (e4m3, per-row scales) form of ``gemm_skinny``: ``y = (res +) (bias +) Q(P(x)) @ Q(w).T`` for 1 <= B <= 64."""
    _chk(x, "x")
    _chk(alpha, "alpha")
    _chk(res, "res")
    _chk(bias, "bias")
    B = x.shape[0]
    N, K = w.shape
    assert x.shape[1] == (2 * K if prologue == PROLOGUE_SILU_GATE else K)
    wp, wsc = skinny_pack_weight_fp8(w)
    b32 = (B + 31) // 32 * 32
    xp = torch.empty(b32, K, device=x.device, dtype=torch.uint8)
    xsc = torch.empty(b32, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_skinny_pack_act_fp8(_ptr(x), _ptr(alpha), _ptr(xp), _ptr(xsc), B, K, x.shape[1], prologue, eps, _stream()))
    out = torch.empty(B, N, device=x.device, dtype=torch.float32)
    with _profiled("gemm_skinny_fp8", 2.0 * B * N * K, N * K + 4 * (x.numel() + out.numel()), (B, N, K)):
        _lib.check(_lib.lib().rst_gemm_skinny_fp8_f32(_ptr(xp), _ptr(xsc), _ptr(wp), _ptr(wsc), _ptr(res), _ptr(bias), _ptr(out), B, N, K, N,
                                                     _stream()))
    return out


def _gemv_route(B: int, K: int) -> bool:
    """The weight-streaming GEMV serves this linear (else the matrix-core skinny GEMM)."""
    return B <= 2 and B * K <= 32768


def _gemv_stored(x: torch.Tensor, w: torch.Tensor, copy, **kw) -> torch.Tensor:
    """One GEMV of the weight-streaming route on the cheapest stored form of ``w`` that serves the shape: an ``Mxfp4Copy`` and
    ``gemv_mxfp4w_supported``, else a plain ``(q, scale)`` fp8 pair and ``gemv_fp8w_supported``, else the bf16 ``w`` itself."""
    B, (N, K) = x.shape[0], w.shape
    if isinstance(copy, Mxfp4Copy):
        if gemv_mxfp4w_supported(B, N, K):
            return gemv_mxfp4w(x, copy[0], copy[1], **kw)
    elif copy is not None and gemv_fp8w_supported(B, N, K):
        return gemv_fp8w(x, copy[0], copy[1], **kw)
    return gemv_bf16(x, w, **kw)


def _skinny_stored(x, w: torch.Tensor, copy, **kw):
    """One skinny GEMM (<= 64 rows) on the cheapest stored form of ``w`` that serves it: a plain ``(q, scale)`` fp8 pair and
    ``gemm_skinny_fp8w_supported``; an opted-in ``Mxfp4BatchedCopy`` and ``gemm_skinny_mxfp4w_supported``; else the bf16 ``w`` itself
    (a plain ``Mxfp4Copy`` keeps the bf16 route above two rows: the batched MXFP4 route is opt-in)."""
    B, (N, K) = x.B if isinstance(x, PackedAct) else x.shape[0], w.shape
    if isinstance(copy, Mxfp4BatchedCopy):
        if gemm_skinny_mxfp4w_supported(B, N, K):
            return gemm_skinny_mxfp4w(x, copy.q, copy.scale, **kw)
    elif copy is not None and not isinstance(copy, Mxfp4Copy) and gemm_skinny_fp8w_supported(B, N, K):
        return gemm_skinny_fp8w(x, copy[0], copy[1], **kw)
    return gemm_skinny(x, w, **kw)


@_on_tensor_device
def lm_gated_pair(x: torch.Tensor, w_in: torch.Tensor, w_out: torch.Tensor, *, alpha: torch.Tensor, eps: float, res: torch.Tensor,
                  bias_in: Optional[torch.Tensor] = None, bias_out: Optional[torch.Tensor] = None, fp8: bool = False,
                  w8_in: Optional[tuple] = None, w8_out: Optional[tuple] = None) -> torch.Tensor:
    """The gated MLP of a decode step: ``res + W_out (silu(u) * v)``, ``[u ; v] = W_in rmsnorm(x)`` (modules/gating.py:12-51,
    lit_model.py:399-403).  Batch <= 2: two GEMVs, the gate in the epilogue of the first (row pairs per wave).  Above: the first skinny GEMM applies
    the gate in its epilogue and hands the packed operand straight to the second -- the gated activation never exists in fp32.
    ``w8_in`` / ``w8_out``: ``(q, scale)`` fp8 copies of the two weights (``quantize_rows_fp8``): the GEMV pair streams them, and so
    does the skinny pair above two rows (``gemm_skinny_fp8w``, the gate in the first epilogue as for bf16).
    Either may instead be an ``Mxfp4Copy`` (``quantize_blocks_mxfp4``): streamed by ``gemv_mxfp4w`` at batch <= 2 only; above, that
    weight is read as bf16 -- unless the copy is an ``Mxfp4BatchedCopy``, which the skinny pair streams too (``gemm_skinny_mxfp4w``)."""
    B = x.shape[0]
    if not fp8 and B <= 2 and B * max(w_out.shape[1], w_in.shape[1]) <= 32768 and w_in.shape[0] % 2 == 0:
        # GEMV pair: every wave of the first owns a (u, v) row pair and writes silu(u) * v; the second is a plain GEMV
        g = _gemv_stored(x, w_in, w8_in, prologue=PROLOGUE_RMSNORM, alpha=alpha, eps=eps, bias=bias_in, gate_out=True)
        return _gemv_stored(g, w_out, w8_out, res=res, bias=bias_out)
    if fp8 or B <= 2 or B > 64 or w_in.shape[0] % 32:
        u = lm_linear(x, w_in, prologue=PROLOGUE_RMSNORM, alpha=alpha, eps=eps, bias=bias_in, fp8=fp8, w8=w8_in)
        return lm_linear(u, w_out, prologue=PROLOGUE_SILU_GATE, res=res, bias=bias_out, fp8=fp8, w8=w8_out)
    g = _skinny_stored(x, w_in, w8_in, prologue=PROLOGUE_RMSNORM, alpha=alpha, eps=eps, bias=bias_in, gate_out=True)
    return _skinny_stored(g, w_out, w8_out, res=res, bias=bias_out)


@_on_tensor_device
def lm_linear(x: torch.Tensor, w: torch.Tensor, *, prologue: int = PROLOGUE_NONE, alpha: Optional[torch.Tensor] = None,
              eps: float = 1e-8, res: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, fp8: bool = False,
              w8: Optional[tuple] = None) -> torch.Tensor:
    """Batch-size dispatch of one decode-step linear: weight-streaming GEMV for B <= 2, bf16-MFMA skinny GEMM above (the
    prologue then runs inside the activation-packing launch).  ``fp8``: the opt-in e4m3 path (any batch <= 64).
    ``w8 = (q, scale)``: an fp8 copy of ``w`` holding the SAME values (``quantize_rows_fp8`` of a weight that was overwritten with its
    dequantised form): the GEMV route streams it instead of ``w``, and so does the skinny route (``gemm_skinny_fp8w``: K % 32 == 0,
    rows above 64 in chunks of 64); the ``fp8=True`` path and unsupported shapes read ``w``.  ``w8`` may instead be an ``Mxfp4Copy``
    (``quantize_blocks_mxfp4``): the GEMV route then streams it with ``gemv_mxfp4w``, every other route reads ``w``; an
    ``Mxfp4BatchedCopy`` is streamed by the skinny route as well (``gemm_skinny_mxfp4w``, same shapes and chunking as fp8)."""
    if isinstance(x, PackedAct):
        return _skinny_stored(x, w, w8, prologue=prologue, res=res, bias=bias)
    if fp8 and x.shape[0] <= 64 and w.shape[1] % 32 == 0 and w.shape[1] <= 16384:
        return gemm_skinny_fp8(x, w, prologue=prologue, alpha=alpha, eps=eps, res=res, bias=bias)
    # the GEMV stages B x K fp32 activations in LDS: beyond two rows that footprint costs occupancy (fewer weight loads in
    # flight) and the matrix-core path is as fast or faster (measured: 4096 x 4096 at B = 3: 16.4 vs 16.5 us, B = 4: 20.9 vs 16.5)
    if _gemv_route(x.shape[0], w.shape[1]):
        return _gemv_stored(x, w, w8, prologue=prologue, alpha=alpha, eps=eps, res=res, bias=bias)
    if x.shape[0] <= 64:
        return _skinny_stored(x, w, w8, prologue=prologue, alpha=alpha, eps=eps, res=res, bias=bias)
    # more rows than one skinny tile set (prompt prefill): chunks of 64 rows, each streaming the weights once
    return torch.cat([_skinny_stored(x[i:i + 64], w, w8, prologue=prologue, alpha=alpha, eps=eps,
                                     res=None if res is None else res[i:i + 64], bias=bias) for i in range(0, x.shape[0], 64)])


def lora_bank_supported(K: int, r: int, N: int) -> bool:
    """Shapes the adapter-bank launches serve (``K % 8 == 0``, ``K <= 16384``, ``r % 16 == 0``, ``r <= 256``, ``N >= 1``); there is no
    other route: ``GPT.load_adapter_bank`` refuses a linear outside them."""
    return bool(_lib.lib().rst_lora_bank_supported(K, r, N))


def _bank_ids(ids: torch.Tensor, rows: int, rows_per_id: int) -> int:
    _chk(ids, "ids", torch.int32)
    if rows_per_id < 1 or rows % rows_per_id or ids.dim() != 1 or ids.numel() != rows // rows_per_id:
        raise ValueError(f"rstnet_amd.ops: {rows} rows are not {ids.numel()} ids x rows_per_id = {rows_per_id}")
    return ids.numel()


@_on_tensor_device
def lora_bank_shrink(x: torch.Tensor, A_bank: torch.Tensor, ids: torch.Tensor, *, rows_per_id: int = 1, prologue: int = PROLOGUE_NONE,
                     alpha: Optional[torch.Tensor] = None, eps: float = 1e-8, post_scale: float = 1.0) -> torch.Tensor:
    """``a[row] = post_scale * A_bank[ids[row // rows_per_id]] @ P(x[row])`` (rst_lora_bank_shrink_f32): ``x`` fp32 ``[rows, K]``
    (``[rows, 2K]`` for the SiLU-gate prologue), ``A_bank`` bf16 ``[n_adapters, r, K]``, ``ids`` int32 ``[rows / rows_per_id]`` on the
    device -> fp32 ``[rows, r]``.  A row whose id is not in ``[0, n_adapters)`` gets zeros.  One summation schedule per element,
    independent of the batch: a row's result does not depend on what it is batched with."""
    _chk(x, "x")
    _chk(A_bank, "A_bank", torch.bfloat16)
    _chk(alpha, "alpha")
    assert x.dim() == 2 and A_bank.dim() == 3, (tuple(x.shape), tuple(A_bank.shape))
    rows = x.shape[0]
    n_ad, r, K = A_bank.shape
    assert x.shape[1] == (2 * K if prologue == PROLOGUE_SILU_GATE else K), (tuple(x.shape), tuple(A_bank.shape), prologue)
    assert alpha is None or alpha.numel() == K, (tuple(alpha.shape), K)
    n_ids = _bank_ids(ids, rows, rows_per_id)
    a = torch.empty(rows, r, device=x.device, dtype=torch.float32)
    with _profiled("lora_bank_shrink", 2.0 * rows * r * K, 2 * min(rows, n_ad) * r * K + 4 * (x.numel() + a.numel()), (rows, r, K)):
        _lib.check(_lib.lib().rst_lora_bank_shrink_f32(_ptr(x), _ptr(alpha), _ptr(A_bank), _ptr(ids), _ptr(a), rows, rows_per_id, n_ids, n_ad,
                                                      r, K, x.shape[1], prologue, eps, post_scale, _stream()))
    return a


@_on_tensor_device
def lora_bank_expand(a: torch.Tensor, B_bank: torch.Tensor, ids: torch.Tensor, y: torch.Tensor, *, rows_per_id: int = 1) -> torch.Tensor:
    """``y[row] += B_bank[ids[row // rows_per_id]] @ a[row]`` IN PLACE (rst_lora_bank_expand_f32): ``a`` fp32 ``[rows, r]``, ``B_bank``
    bf16 ``[n_adapters, N, r]``, ``y`` fp32 ``[rows, N]``; returns ``y``.  A row whose id is not in ``[0, n_adapters)`` keeps its bits."""
    _chk(a, "a")
    _chk(B_bank, "B_bank", torch.bfloat16)
    _chk(y, "y")
    assert a.dim() == 2 and B_bank.dim() == 3 and y.dim() == 2, (tuple(a.shape), tuple(B_bank.shape), tuple(y.shape))
    rows = a.shape[0]
    n_ad, N, r = B_bank.shape
    assert a.shape[1] == r and tuple(y.shape) == (rows, N), (tuple(a.shape), tuple(B_bank.shape), tuple(y.shape))
    n_ids = _bank_ids(ids, rows, rows_per_id)
    with _profiled("lora_bank_expand", 2.0 * rows * r * N, 2 * min(rows, n_ad) * r * N + 4 * (a.numel() + 2 * y.numel()), (rows, N, r)):
        _lib.check(_lib.lib().rst_lora_bank_expand_f32(_ptr(a), _ptr(B_bank), _ptr(ids), _ptr(y), rows, rows_per_id, n_ids, n_ad, N, r, N,
                                                      _stream()))
    return y


@_on_tensor_device
def embed_sum(tokens: torch.Tensor, tables: Sequence[torch.Tensor], tok_index: Sequence[int],
              add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[b] = (add[b] +) sum_i tables[i][tokens[b, tok_index[i]]]``; tokens int64 ``[B, n]`` (rows contiguous, any row stride), tables
    bf16 ``[rows, D]``; ``add`` fp32 ``[B, D]`` with unit column stride and any row stride (a column block of a wider matrix is read in place)."""
    _chk(tokens, "tokens", torch.int64, contiguous=False)
    if add is not None:
        _chk(add, "add", contiguous=False)
        assert add.dim() == 2 and add.stride(1) == 1, "embed_sum: `add` needs unit column stride"
    assert tokens.dim() == 2 and tokens.stride(1) == 1, "embed_sum: `tokens` needs unit column stride"
    for t in tables:
        _chk(t, "table", torch.bfloat16)
    B, D = tokens.shape[0], tables[0].shape[1]
    out = torch.empty(B, D, device=tokens.device, dtype=torch.float32)
    tabs = (C.c_void_p * len(tables))(*[t.data_ptr() for t in tables])
    _lib.check(_lib.lib().rst_embed_sum_bf16(_ptr(tokens), tabs, _int_array(list(tok_index)), _int_array([t.shape[0] for t in tables]),
                                            len(tables), _ptr(add), _ptr(out), B, D, tokens.stride(0), add.stride(0) if add is not None else D,
                                            _stream()))
    return out


@_on_tensor_device
def rmsnorm(x: torch.Tensor, alpha: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    _chk(x, "x")
    _chk(alpha, "alpha")
    out = torch.empty_like(x)
    _lib.check(_lib.lib().rst_rmsnorm_f32(_ptr(x), _ptr(alpha), _ptr(out), x.numel() // x.shape[-1], x.shape[-1], eps, _stream()))
    return out


# Workgroups a (stream, head) pair's ring is split over in the single-step decode attention (rst_lm_attn_decode_f32): at most this many,
# at least 128 slots each, ~1024 workgroups per launch (the A/B switch of tools/ab.py).
LM_ATTN_MAX_SPLITS = 16


def lm_attn_splits(cap: int, pairs: int) -> int:
    return max(1, min(int(LM_ATTN_MAX_SPLITS), cap // 128, 1024 // max(1, pairs)))


@_on_tensor_device
def lm_rope_append(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos_dev: torch.Tensor, *, heads: int, rope: bool,
                   max_period: float = 10000.0, rope_dims: int = 0) -> torch.Tensor:
    """qkv ``[B, T, (H+2G)*D]`` (T new steps) -> rotated q ``[B, H, T, D]``; k/v appended to ring slots ``(pos+t) % cap`` of
    ``[B,G,cap,D]``.  ``rope_dims``: leading head dims that rotate (0 = all)."""
    for t, n in ((qkv, "qkv"), (k_cache, "k_cache"), (v_cache, "v_cache")):
        _chk(t, n)
    _chk(pos_dev, "pos_dev", torch.int64)
    _shared_pos(pos_dev, "lm_rope_append")
    B, G, cap, D = k_cache.shape
    T = qkv.shape[1]
    assert qkv.dim() == 3 and qkv.shape[2] == (heads + 2 * G) * D, (tuple(qkv.shape), heads, G, D)
    q = torch.empty(B, heads, T, D, device=qkv.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_lm_rope_append_f32(_ptr(qkv), _ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(pos_dev), B, T, heads, G, D, cap,
                                                qkv.shape[2], int(rope), rope_coef(max_period, rope_dims or D), rope_dims, _stream()))
    return q


@_on_tensor_device
def lm_rope_table(pos_dev: torch.Tensor, D: int, *, max_period: float = 10000.0, rope_dims: int = 0) -> torch.Tensor:
    """The rotation of ONE decode step as ``[D/2, 2]`` (cos, sin) pairs (rst_lm_rope_table_f32; identity beyond ``rope_dims / 2``): computed
    once per frame and handed to every layer's ``lm_attn_decode(rope_table=...)`` -- the values the attention launch would compute itself.
    Per-stream positions (``pos_dev`` int64 ``[B]``, a 1-D vector of more than one element): ``[B, D/2, 2]``, table ``b`` at ``pos_dev[b]``
    (rst_lm_rope_table_ps_f32)."""
    _chk(pos_dev, "pos_dev", torch.int64)
    if pos_dev.numel() == 1:
        out = torch.empty(D // 2, 2, device=pos_dev.device, dtype=torch.float32)
        _lib.check(_lib.lib().rst_lm_rope_table_f32(_ptr(pos_dev), _ptr(out), D, rope_dims, rope_coef(max_period, rope_dims or D), _stream()))
        return out
    B = pos_dev.numel()
    _pos_stride(pos_dev, B, "lm_rope_table")
    out = torch.empty(B, D // 2, 2, device=pos_dev.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_lm_rope_table_ps_f32(_ptr(pos_dev), _ptr(out), B, D, rope_dims, rope_coef(max_period, rope_dims or D), _stream()))
    return out


@_on_tensor_device
def lm_attn_decode(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos_dev: torch.Tensor, *, rope: bool,
                   context: Optional[int], max_period: float = 10000.0, splits: Optional[int] = None,
                   scratch: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, heads: Optional[int] = None,
                   rope_dims: int = 0, packed: bool = False, rope_table: Optional[torch.Tensor] = None):
    """Single-query attention of the new step given its qkv row ``[B, (H+2G)*D]`` (RoPE, ring append, attention and the
    reduction over slot splits in ONE launch) -> ``[B, H*D]``; the ring is ``[B,G,cap,D]`` (``heads`` = H when G < H).
    ``scratch = (ws [B,H,splits,D+2] fp32, counters [B,H] int32 zeros)`` may be passed to reuse buffers (the counters re-arm
    themselves).  ``rope_dims``: leading head dims that rotate (0 = all; the frequencies then span ``rope_dims``).  ``pos_dev``: one
    position for all streams (``numel() == 1``, rst_lm_attn_decode_f32) or int64 ``[B]``, one per stream (rst_lm_attn_decode_ps_f32;
    ``rope_table`` is then the ``[B, D/2, 2]`` table ``lm_rope_table`` returns for that vector)."""
    _chk(qkv, "qkv")
    kv16 = k_cache.dtype == torch.bfloat16          # bf16 rings: the reference's cache precision (long-ring form)
    _chk(k_cache, "k_cache", k_cache.dtype if kv16 else torch.float32)
    _chk(v_cache, "v_cache", k_cache.dtype)
    _chk(pos_dev, "pos_dev", torch.int64)
    _chk(rope_table, "rope_table")
    B, G, cap, D = k_cache.shape
    H = heads or G
    assert qkv.shape[1] == (H + 2 * G) * D, (tuple(qkv.shape), H, G, D)
    ps = _pos_stride(pos_dev, B, "lm_attn_decode")
    assert rope_table is None or rope_table.numel() == (B * D if ps else D), "rope_table: what lm_rope_table returns for this pos_dev"
    if kv16 and cap <= 64:
        raise NotImplementedError("bf16 KV rings are served by the long-ring attention (capacity > 64)")
    if splits is None:
        splits = 1 if cap <= 64 else lm_attn_splits(cap, B * H)
    ws = counters = None
    if splits > 1:
        if scratch is None:
            scratch = (torch.empty(B, H, splits, D + 2, device=qkv.device, dtype=torch.float32),
                       torch.zeros(B, H, device=qkv.device, dtype=torch.int32))
        ws, counters = scratch
        _chk(ws, "ws"); _chk(counters, "counters", torch.int32)
        assert ws.numel() >= B * H * splits * (D + 2) and counters.numel() >= B * H
    # packed=True (head dim 64 / 128): the result leaves as the bf16 hi / lo operand of the out-projection's skinny GEMM
    packed = packed and D in (64, 128)
    out = None if packed else torch.empty(B, H * D, device=qkv.device, dtype=torch.float32)
    xp = _packed_buffer(qkv.device, B, H * D) if packed else None
    head = (_ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(ws), _ptr(counters), _ptr(out), _ptr(pos_dev))
    tail = (B, H, D, cap, _ctx(context), splits, qkv.shape[1], int(rope), rope_coef(max_period, rope_dims or D), G, rope_dims, _ptr(xp), int(kv16),
            _ptr(rope_table) if rope else None, _stream())
    _lib.check(_lib.lib().rst_lm_attn_decode_ps_f32(*head, ps, *tail) if ps else _lib.lib().rst_lm_attn_decode_f32(*head, *tail))
    return PackedAct(xp, B, H * D) if packed else out


_prefill_ws: dict = {}
_rope_freq_tables: dict = {}


def _rope_freqs(device, max_period: float, n: int) -> torch.Tensor:
    """The reference's frequency table ``exp(arange(n / 2) * (-ln(max_period) * 2 / n))`` (modules/rope.py:37-38) evaluated as the
    reference writes it, by torch in fp32, once per (device, max_period, n).  The prefill kernels multiply it by positions in the
    thousands, where one ulp of a frequency is 2e-4 rad: the table keeps the stored keys on the reference's angles."""
    key = (device, float(max_period), n)
    tab = _rope_freq_tables.get(key)
    if tab is None:
        ds = torch.arange(n // 2, dtype=torch.float32)
        tab = _rope_freq_tables[key] = torch.exp(ds * (-math.log(max_period) * 2 / n)).to(device)
    return tab


def gpt_rope_freqs(device, base: float, n: int) -> torch.Tensor:
    """litgpt's frequency table ``1 / base ** (arange(0, n, 2) / n)`` (lit_model.build_rope_cache) evaluated as that reference writes
    it, by torch in fp32, once per (device, base, n): the table ``GPT`` hands to ``lm_attn_prefill`` / ``lm_ring_append`` as ``freqs``."""
    key = ("gpt", device, float(base), n)
    tab = _rope_freq_tables.get(key)
    if tab is None:
        tab = _rope_freq_tables[key] = (1.0 / (base ** (torch.arange(0, n, 2).float() / n))).to(device)
    return tab


def _prefill_args(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos_dev: torch.Tensor, heads: Optional[int],
                  freqs: Optional[torch.Tensor], rope_dims: int):
    _chk(qkv, "qkv")
    kv16 = k_cache.dtype == torch.bfloat16
    _chk(k_cache, "k_cache", k_cache.dtype if kv16 else torch.float32)
    _chk(v_cache, "v_cache", k_cache.dtype)
    _chk(pos_dev, "pos_dev", torch.int64)
    _chk(freqs, "freqs")
    B, G, cap, D = k_cache.shape
    H = heads or G
    assert qkv.dim() == 3 and qkv.shape[0] == B and qkv.shape[2] == (H + 2 * G) * D, (tuple(qkv.shape), B, H, G, D)
    assert v_cache.shape == k_cache.shape
    assert freqs is None or freqs.numel() >= (rope_dims or D) // 2, "freqs: one frequency per rotating pair"
    return B, qkv.shape[1], H, G, D, cap, kv16


@_on_tensor_device
def lm_attn_prefill(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos_dev: torch.Tensor, *, window: int,
                    rope: bool, max_period: float = 10000.0, rope_dims: int = 0, heads: Optional[int] = None,
                    freqs: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention of ``Tc`` new positions given their in-projection ``qkv [B, Tc, (H+2G)*D]`` against the ring ``[B,G,cap,D]`` (bf16 or
    fp32) plus the chunk itself, BEFORE anything is appended -> ``[B*Tc, H*D]``.  The query at position ``p`` (``pos_dev`` = position of
    row 0) sees keys ``max(0, p - window + 1) .. p``; the chunk's own keys / values take part rounded to the ring's dtype.  Follow with
    ``lm_ring_append`` (head dim 64 / 128, ``Tc <= cap``, ``1 <= window <= cap``).  ``heads`` = H when the ring holds G < H grouped
    key/value heads (as in ``lm_attn_decode``; None: G == H, rst_lm_attn_prefill_f32, else rst_lm_attn_prefill_gqa_f32).  ``freqs``: the
    fp32 frequency table of the caller's reference (``rope_dims / 2`` values); None: the Moshi table of ``_rope_freqs``.  ``pos_dev`` int64
    ``[B]``: the chunk of stream ``b`` starts at ``pos_dev[b]`` (rst_lm_attn_prefill_ps_f32)."""
    B, Tc, H, G, D, cap, kv16 = _prefill_args(qkv, k_cache, v_cache, pos_dev, heads, freqs, rope_dims)
    ps = _pos_stride(pos_dev, B, "lm_attn_prefill")
    L = _lib.lib()
    nbytes = int(L.rst_lm_attn_prefill_workspace_bytes(B, Tc, H, D, int(kv16)) if heads is None else
                 L.rst_lm_attn_prefill_gqa_workspace_bytes(B, Tc, H, G, D, int(kv16)))
    if nbytes <= 0:
        raise ValueError(f"rstnet_amd.ops: lm_attn_prefill workspace for B={B} Tc={Tc} H={H} G={G} D={D} is not addressable")
    ws = _scratch(_prefill_ws, qkv.device, ("prefill", nbytes), lambda: torch.empty((nbytes + 7) // 8, device=qkv.device, dtype=torch.int64))
    out = torch.empty(B * Tc, H * D, device=qkv.device, dtype=torch.float32)
    if freqs is None:
        freqs = _rope_freqs(qkv.device, max_period, rope_dims or D)
    head = (_ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(ws), nbytes, _ptr(out), _ptr(pos_dev))
    tail = (D, cap, int(window), qkv.shape[2], int(rope), rope_coef(max_period, rope_dims or D), rope_dims, int(kv16),
            _ptr(freqs) if rope else None, _stream())
    if ps:
        _lib.check(L.rst_lm_attn_prefill_ps_f32(*head, ps, B, Tc, H, G, *tail))
    else:
        _lib.check(L.rst_lm_attn_prefill_f32(*head, B, Tc, H, *tail) if heads is None else L.rst_lm_attn_prefill_gqa_f32(*head, B, Tc, H, G, *tail))
    return out


@_on_tensor_device
def lm_ring_append(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos_dev: torch.Tensor, *, rope: bool,
                   max_period: float = 10000.0, rope_dims: int = 0, heads: Optional[int] = None,
                   freqs: Optional[torch.Tensor] = None) -> None:
    """The append that follows ``lm_attn_prefill`` in stream order: the ``Tc`` keys of ``qkv [B, Tc, (H+2G)*D]`` rotated at positions
    ``pos_dev + t``, and the values, into ring slots ``(pos_dev + t) % cap`` of ``[B,G,cap,D]`` in the ring's dtype (rst_lm_ring_append;
    ``heads`` given: rst_lm_ring_append_gqa).  ``heads`` / ``freqs`` as in ``lm_attn_prefill``.  ``pos_dev`` int64 ``[B]``: per-stream
    positions (rst_lm_ring_append_ps).  Per-stream LENGTHS: ``lm_ring_append_ragged``."""
    _ring_append(qkv, k_cache, v_cache, pos_dev, rope, max_period, rope_dims, heads, freqs, None, 0)


@_on_tensor_device
def lm_ring_append_ragged(qkv: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos_dev: torch.Tensor, *, rope: bool,
                          max_period: float = 10000.0, rope_dims: int = 0, heads: Optional[int] = None,
                          freqs: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None, t0: int = 0) -> None:
    """``lm_ring_append`` with per-stream lengths (rst_lm_ring_append_ps): ``lengths`` int32 ``[B]`` on the device with the offset ``t0`` of
    this chunk inside the call the lengths count from -- stream ``b`` appends rows ``t < clamp(lengths[b] - t0, 0, Tc)`` only and no other
    ring slot is written; a length of 0 takes nothing.  ``pos_dev``: one position or int64 ``[B]``.  (Its own entry point so that
    ``lm_ring_append`` keeps the signature its callers and their recorded launch plans know.)"""
    _ring_append(qkv, k_cache, v_cache, pos_dev, rope, max_period, rope_dims, heads, freqs, lengths, t0)


def _ring_append(qkv, k_cache, v_cache, pos_dev, rope, max_period, rope_dims, heads, freqs, lengths, t0) -> None:
    B, Tc, H, G, D, cap, kv16 = _prefill_args(qkv, k_cache, v_cache, pos_dev, heads, freqs, rope_dims)
    ps = _pos_stride(pos_dev, B, "lm_ring_append")
    _chk(lengths, "lengths", torch.int32)
    if lengths is not None and (lengths.dim() != 1 or lengths.numel() != B):
        raise ValueError(f"rstnet_amd.ops: lm_ring_append: lengths must be int32 [{B}], got {tuple(lengths.shape)}")
    if t0 < 0:
        raise ValueError(f"rstnet_amd.ops: lm_ring_append: chunk offset t0 = {t0}")
    L = _lib.lib()
    if freqs is None:
        freqs = _rope_freqs(qkv.device, max_period, rope_dims or D)
    head = (_ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(pos_dev))
    tail = (D, cap, qkv.shape[2], int(rope), rope_coef(max_period, rope_dims or D), rope_dims, int(kv16), _ptr(freqs) if rope else None,
            _stream())
    if ps or lengths is not None:
        _lib.check(L.rst_lm_ring_append_ps(*head, ps, _ptr(lengths), int(t0), B, Tc, H, G, *tail))
    else:
        _lib.check(L.rst_lm_ring_append(*head, B, Tc, H, *tail) if heads is None else L.rst_lm_ring_append_gqa(*head, B, Tc, H, G, *tail))


_sample_ws: dict = {}


@_on_tensor_device
def lm_sample(logits: torch.Tensor, *, use_sampling: bool, temp: float, top_k: int, noise: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, limit: int = 0, limit_dev: Optional[torch.Tensor] = None, top_p: float = 0.0,
              two_level: bool = True) -> torch.Tensor:
    """logits fp32 ``[B, V]`` -> tokens int64 ``[B]`` (greedy, or top-k sampling with Exp(1) ``noise [B, top_k]``).  ``limit``
    (or the int32 device scalar ``limit_dev``; int32 ``[B]``, any element stride, e.g. a column of a ``[B, n]`` table: one limit per row,
    rst_lm_sample_rows_f32): ids >= limit are never drawn when sampling.  ``top_p > 0``: nucleus sampling
    (utils/sampling.py:66-82) instead of top-k; ``noise`` is then ``[B, V]`` (one draw per sorted position).  ``two_level=False``
    keeps the one-workgroup-per-row kernel for vocabularies above 32768 (A/B measurements, tests).  One temperature and top-k per row:
    ``lm_sample_ps``."""
    _chk(logits, "logits")
    _chk(limit_dev, "limit_dev", torch.int32, contiguous=False)
    B, V = logits.shape
    if limit_dev is not None and limit_dev.numel() != 1 and (limit_dev.dim() != 1 or limit_dev.numel() != B):
        raise ValueError(f"rstnet_amd.ops: `limit_dev` holds one limit, or one per row as int32 [{B}]; got {tuple(limit_dev.shape)}")
    rows = limit_dev is not None and limit_dev.numel() == B and B > 1
    sampling = bool(use_sampling and temp > 0)
    nucleus = sampling and top_p > 0.0
    if noise is not None:       # a [B, >= top_k] column slice of a wider noise buffer is fine (row stride is passed on)
        if not noise.is_cuda or noise.dtype != torch.float32 or noise.dim() != 2 or noise.stride(1) != 1 or noise.shape[0] != B:
            raise ValueError("rstnet_amd.ops: `noise` must be a float32 CUDA/HIP tensor [B, k] with unit column stride")
        if nucleus and noise.shape[1] < V:
            raise ValueError(f"rstnet_amd.ops: top_p sampling draws one noise value per vocabulary entry: noise [B, >= {V}] needed")
    if out is None:
        out = torch.empty(B, device=logits.device, dtype=torch.int64)
    elif not out.is_cuda or out.dtype != torch.int64 or out.dim() != 1 or out.shape[0] != B:   # may be a column of a [B, n] buffer
        raise ValueError("rstnet_amd.ops: `out` must be an int64 CUDA/HIP vector of length B")
    ws, nbytes = None, 0
    if nucleus or (two_level and V > 32768):
        nbytes = int(_lib.lib().rst_lm_sample_workspace_bytes(B, V, top_k if sampling else 1, int(nucleus)))
        if nbytes:
            ws = _scratch(_sample_ws, logits.device, ("sample", nbytes), lambda: torch.empty((nbytes + 7) // 8, device=logits.device, dtype=torch.int64))
    head = (_ptr(logits), _ptr(noise), _ptr(out), B, V, V, top_k, noise.stride(0) if noise is not None else 0, out.stride(0) if B > 1 else 1,
            int(use_sampling), float(temp), int(limit), _ptr(limit_dev))
    tail = (float(top_p) if nucleus else 0.0, _ptr(ws), nbytes, _stream())
    _lib.check(_lib.lib().rst_lm_sample_rows_f32(*head, limit_dev.stride(0), *tail) if rows else _lib.lib().rst_lm_sample_f32(*head, *tail))
    return out


@_on_tensor_device
def lm_sample_ps(logits: torch.Tensor, *, top_k: int, noise: Optional[torch.Tensor], temps: Optional[torch.Tensor],
                 top_ks: Optional[torch.Tensor], out: Optional[torch.Tensor] = None, limit: int = 0,
                 limit_dev: Optional[torch.Tensor] = None, top_p: float = 0.0) -> torch.Tensor:
    """``lm_sample`` with one temperature and one top-k per row (rst_lm_sample_ps_f32): ``temps`` fp32 ``[B]`` (<= 0: that
    row is greedy and reads no noise) with ``top_ks`` int32 ``[B]``, device tensors of one common element stride (e.g. two columns of
    ``[B, n]`` tables).  ``top_k`` is the CAP: the kernel clamps every row's value into 1 .. cap, and ``noise`` is ``[B, >= cap]``.  Served by the
    one-level top-k kernel only; refused, never substituted: ``top_p > 0`` and V > 32768.  (Its own entry point so that ``lm_sample`` keeps
    the signature its callers and their recorded launch plans know.)"""
    _chk(logits, "logits")
    _chk(limit_dev, "limit_dev", torch.int32, contiguous=False)
    B, V = logits.shape
    if temps is None or top_ks is None:
        raise ValueError("rstnet_amd.ops: lm_sample: per-row parameters come as a pair, `temps` fp32 [B] and `top_ks` int32 [B]")
    _chk(temps, "temps", torch.float32, contiguous=False)
    _chk(top_ks, "top_ks", torch.int32, contiguous=False)
    if temps.dim() != 1 or top_ks.dim() != 1 or temps.numel() != B or top_ks.numel() != B:
        raise ValueError(f"rstnet_amd.ops: lm_sample: `temps` / `top_ks` hold one value per row ([{B}]); got {tuple(temps.shape)} / {tuple(top_ks.shape)}")
    stride = temps.stride(0) if B > 1 else 1
    if B > 1 and top_ks.stride(0) != stride:
        raise ValueError(f"rstnet_amd.ops: lm_sample: `temps` and `top_ks` need one common element stride, got {temps.stride(0)} and {top_ks.stride(0)}")
    if top_p > 0.0:
        raise ValueError("rstnet_amd.ops: lm_sample: per-row parameters are not served with top_p > 0 (nucleus sampling keeps scalar parameters)")
    if V > 32768:
        raise ValueError(f"rstnet_amd.ops: lm_sample: per-row parameters are served by the one-level kernel only (V <= 32768), got V = {V}")
    cap = min(int(top_k), V)
    if cap < 1:
        raise ValueError(f"rstnet_amd.ops: lm_sample: with per-row parameters `top_k` is the cap of every row's top-k: >= 1, got {top_k}")
    if noise is None or not noise.is_cuda or noise.dtype != torch.float32 or noise.dim() != 2 or noise.stride(1) != 1 \
            or noise.shape[0] != B or noise.shape[1] < cap:
        raise ValueError(f"rstnet_amd.ops: lm_sample: per-row parameters need `noise` float32 [B, >= {cap}] with unit column stride")
    if limit_dev is not None and limit_dev.numel() != 1 and (limit_dev.dim() != 1 or limit_dev.numel() != B):
        raise ValueError(f"rstnet_amd.ops: `limit_dev` holds one limit, or one per row as int32 [{B}]; got {tuple(limit_dev.shape)}")
    if out is None:
        out = torch.empty(B, device=logits.device, dtype=torch.int64)
    elif not out.is_cuda or out.dtype != torch.int64 or out.dim() != 1 or out.shape[0] != B:
        raise ValueError("rstnet_amd.ops: `out` must be an int64 CUDA/HIP vector of length B")
    rows = limit_dev is not None and limit_dev.numel() == B and B > 1
    _lib.check(_lib.lib().rst_lm_sample_ps_f32(
        _ptr(logits), _ptr(noise), _ptr(out), B, V, V, cap, noise.stride(0), out.stride(0) if B > 1 else 1, 1, 1.0, int(limit), _ptr(limit_dev),
        limit_dev.stride(0) if rows else 0, 0.0, None, 0, _stream(), _ptr(temps), _ptr(top_ks), stride))
    return out


@_on_tensor_device
def noise_exp_rows(seeds: torch.Tensor, frames: torch.Tensor, n_cols: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exp(1) noise fp32 ``[B, n_cols]`` for the samplers as a counter-based stream (rst_noise_exp_ps_f32): row ``b``
    is a pure function of ``seeds[b]`` (int64 ``[B]``, read as uint64), its frame counter -- ``frames`` int64 ``[B]``, or one element for
    the whole batch -- and the column.  Both are read from device memory by the launch.  ``out``: fp32 ``[B, >= n_cols]`` with unit column
    stride (columns past ``n_cols`` are left alone); returns the ``[B, n_cols]`` view."""
    _chk(seeds, "seeds", torch.int64)
    _chk(frames, "frames", torch.int64)
    if seeds.dim() != 1 or seeds.numel() < 1:
        raise ValueError(f"rstnet_amd.ops: noise_exp_rows: `seeds` is int64 [B], got {tuple(seeds.shape)}")
    B = seeds.numel()
    if frames.numel() not in (1, B):
        raise ValueError(f"rstnet_amd.ops: noise_exp_rows: `frames` holds one counter, or one per row as int64 [{B}]; got {tuple(frames.shape)}")
    n_cols = int(n_cols)
    if n_cols < 1:
        raise ValueError(f"rstnet_amd.ops: noise_exp_rows: n_cols = {n_cols}")
    if out is None:
        out = torch.empty(B, n_cols, device=seeds.device, dtype=torch.float32)
    elif not out.is_cuda or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < n_cols or out.stride(1) != 1 \
            or (B > 1 and out.stride(0) < n_cols):
        raise ValueError(f"rstnet_amd.ops: noise_exp_rows: `out` must be float32 [{B}, >= {n_cols}] with unit column stride")
    with _profiled("noise_exp", 0.0, 4 * B * n_cols + 16 * B, (B, n_cols)):
        _lib.check(_lib.lib().rst_noise_exp_ps_f32(_ptr(out), B, n_cols, out.stride(0) if B > 1 else max(out.stride(0), n_cols), _ptr(seeds),
                                                  _ptr(frames), 1 if frames.numel() == B and B > 1 else 0, _stream()))
    return out[:, :n_cols]


@_on_tensor_device
def lm_ring_begin(cache: torch.Tensor, user_tokens: torch.Tensor, initial: torch.Tensor, delays: torch.Tensor,
                  offset_dev: torch.Tensor, first_user_k: int) -> torch.Tensor:
    """Start of an ``LMGen.step`` frame on the device (models/model.py:506-521): user streams into the token ring
    ``cache [B, K, CT]`` at their delayed columns, initial tokens while ``offset <= delay``; returns the model input ``[B, K]``.
    ``offset_dev``: the one frame counter of the batch (``numel() == 1``) or int64 ``[B]``, one per stream (rst_lm_ring_begin_ps_i64)."""
    for t, n in ((cache, "cache"), (user_tokens, "user_tokens"), (initial, "initial"), (offset_dev, "offset_dev")):
        _chk(t, n, torch.int64)
    _chk(delays, "delays", torch.int32)
    B, K, CT = cache.shape
    Ki = user_tokens.shape[1]
    assert user_tokens.shape[0] == B and initial.numel() == K and delays.numel() == K
    out = torch.empty(B, K, device=cache.device, dtype=torch.int64)
    if _pos_stride(offset_dev, B, "lm_ring_begin"):
        _lib.check(_lib.lib().rst_lm_ring_begin_ps_i64(_ptr(cache), _ptr(user_tokens), _ptr(initial), _ptr(delays), _ptr(offset_dev), 1, _ptr(out),
                                                      B, K, CT, Ki, first_user_k, _stream()))
        return out
    _lib.check(_lib.lib().rst_lm_ring_begin_i64(_ptr(cache), _ptr(user_tokens), _ptr(initial), _ptr(delays), _ptr(offset_dev), _ptr(out),
                                               B, K, CT, Ki, first_user_k, _stream()))
    return out


@_on_tensor_device
def lm_ring_commit(cache: torch.Tensor, tokens: torch.Tensor, delays: torch.Tensor, offset_dev: torch.Tensor, max_delay: int) -> torch.Tensor:
    """End of the frame (models/model.py:545-562): ``offset_dev += 1``, generated ``tokens [B, n]`` into the ring, returns the
    delay-aligned gather ``[B, n]`` (meaningful once ``offset > max_delay``).  ``offset_dev`` int64 ``[B]``: one counter per stream, each
    incremented (rst_lm_ring_commit_ps_i64); row ``b`` is meaningful once ITS counter exceeds ``max_delay``."""
    for t, n in ((cache, "cache"), (tokens, "tokens"), (offset_dev, "offset_dev")):
        _chk(t, n, torch.int64)
    _chk(delays, "delays", torch.int32)
    B, K, CT = cache.shape
    n_out = tokens.shape[1]
    out = torch.empty(B, n_out, device=cache.device, dtype=torch.int64)
    if _pos_stride(offset_dev, B, "lm_ring_commit"):
        _lib.check(_lib.lib().rst_lm_ring_commit_ps_i64(_ptr(cache), _ptr(tokens), _ptr(delays), _ptr(offset_dev), 1, _ptr(out), B, K, CT, n_out,
                                                       int(max_delay), _stream()))
        return out
    _lib.check(_lib.lib().rst_lm_ring_commit_i64(_ptr(cache), _ptr(tokens), _ptr(delays), _ptr(offset_dev), _ptr(out), B, K, CT, n_out,
                                                int(max_delay), _stream()))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# The three persistent frame launches (csrc/persist.h): the depth phase, the batch-1 temporal transformer, a Mimi transformer step
# ----------------------------------------------------------------------------------------------------------------------
def _device_index(device=None) -> int:
    """Ordinal of ``device`` (a torch device / int / None = the current device): the key of every per-device cache."""
    if device is None:
        return torch.cuda.current_device()
    d = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    return d.index if d.index is not None else torch.cuda.current_device()


@functools.lru_cache(maxsize=512)
def _frame_grid(entry: str, dev: int, *shape: int) -> int:
    """Workgroups the library's ``entry`` (an ``rst_*_supported``) grants ``shape`` on device ``dev``, 0 = not served.  Keyed by the
    device ordinal and asked with that device current: the answer embeds its CU count and its occupancy query."""
    with torch.cuda.device(dev):
        return int(getattr(_lib.lib(), entry)(*shape))


_frame_ws: dict = {"depth_frame": {}, "temporal_frame": {}, "codec_transformer": {}}          # kind -> `_scratch` cache
_depth_ws, _temporal_ws = _frame_ws["depth_frame"], _frame_ws["temporal_frame"]          # read by the test helpers of earlier revisions


def _frame_workspace(kind: str, device, shape: tuple) -> torch.Tensor:
    """The granule workspace (int64 words, ``rst_<kind>_workspace_bytes(*shape)``) of a persistent launcher, through `_scratch`."""
    return _scratch(_frame_ws[kind], device, shape,
                    lambda: torch.zeros(int(getattr(_lib.lib(), f"rst_{kind}_workspace_bytes")(*shape)) // 8, device=device, dtype=torch.int64))


def frame_workspace(kind: str, shape: tuple, device=None) -> Optional[torch.Tensor]:
    """The workspace an EAGER launch of ``kind`` ("depth_frame": ``(B, E, Hd, card)``, "temporal_frame": ``(E, Hd, H)``,
    "codec_transformer": ``(rows, E, F)``) used for ``shape`` on ``device``, None before the first one (tests read the hand-offs)."""
    dev = _device_index(device)
    return next((ws for k, ws in _frame_ws[kind].items() if k[0].index == dev and k[1] != "graph" and k[2:] == tuple(shape)), None)


# ---- the depth phase of a frame (rst_depth_decode_frame) ---------------------------------------------------------------------------------
DEPTH_FRAME_MAX_L, DEPTH_FRAME_MAX_Q = 8, 8


def depth_frame_supported(B: int, E: int, H: int, Hd: int, card: int, dep_q: int, L: int, top_k: int, device=None) -> bool:
    """Shapes ``rst_depth_decode_frame`` serves -- the library's own answer (rst_depth_frame_supported: batch 1 / 2, E and Hd multiples
    of 8, card <= 4096, at most 8 layers and 8 steps, the LDS footprint, a grid in which every workgroup owns rows of every
    all-to-all op and that still has a workgroup per head, and the occupancy query), so that callers can pick the per-op path
    instead of catching an error."""
    if not (1 <= B <= 2 and 1 <= dep_q <= DEPTH_FRAME_MAX_Q and 1 <= L <= DEPTH_FRAME_MAX_L and H >= 1 and E % max(H, 1) == 0):
        return False
    return _frame_grid("rst_depth_frame_supported", _device_index(device), B, E, H, Hd, card, dep_q, L, top_k if 0 < top_k < card else card) > 0


@_on_tensor_device
def depth_decode_frame(tables, h_all: torch.Tensor, tokens: torch.Tensor, noise: Optional[torch.Tensor], *, use_sampling: bool,
                       temp: float, top_k: int, eps: float, context: Optional[int] = None, limits: Optional[torch.Tensor] = None,
                       ring_cap: Optional[int] = None) -> None:
    """``tables``: a ``lm.depth_frame.DepthFrameTables``; ``h_all`` fp32 ``[B, dep_q * E]``; ``tokens`` int64 ``[B, >= dep_q + 1]`` with the
    text token in column 0 -- columns 1 .. dep_q are written; ``noise`` fp32 ``[B, >= dep_q * top_k]`` (unit column stride);
    ``limits`` int32 ``[dep_q]`` on the device (optional id blanking per step), or ``[B, dep_q]``: one row of limits per stream
    (rst_depth_decode_frame_rows); ``ring_cap``: capacity of the depth transformer's KV
    ring (default dep_q, the LMGen setup; the slot -> position map of RingKVCache.complete depends on it)."""
    _chk(h_all, "h_all")
    _chk(limits, "limits", torch.int32)
    if not tokens.is_cuda or tokens.dtype != torch.int64 or tokens.dim() != 2 or tokens.stride(1) != 1:
        raise ValueError("rstnet_amd.ops: `tokens` must be an int64 CUDA/HIP matrix with unit column stride")
    B = h_all.shape[0]
    t = tables
    assert h_all.shape[1] == t.dep_q * t.E and tokens.shape[0] == B and tokens.shape[1] >= t.dep_q + 1
    if limits is not None and not (limits.dim() == 1 and limits.numel() >= t.dep_q) and \
            not (limits.dim() == 2 and limits.shape[0] == B and limits.shape[1] >= t.dep_q):
        raise ValueError(f"rstnet_amd.ops: `limits` must be int32 [>= {t.dep_q}] or [{B}, >= {t.dep_q}], got {tuple(limits.shape)}")
    fn, lim = _lib.lib().rst_depth_decode_frame, (_ptr(limits),)
    if limits is not None and limits.dim() == 2:
        fn, lim = _lib.lib().rst_depth_decode_frame_rows, (_ptr(limits), limits.shape[1])
    sampling = bool(use_sampling and temp > 0)
    if sampling:
        if noise is None or not noise.is_cuda or noise.dtype != torch.float32 or noise.dim() != 2 or noise.stride(1) != 1 or \
                noise.shape[0] != B or noise.shape[1] < t.dep_q * top_k:
            raise ValueError("rstnet_amd.ops: `noise` must be float32 CUDA/HIP [B, >= dep_q * top_k] with unit column stride")
    ws = _frame_workspace("depth_frame", h_all.device, (B, t.E, t.Hd, t.card))
    n_w = t.dep_q * (t.L * (3 * t.E * t.E + t.E * t.E + 3 * t.Hd * t.E) + t.card * t.E)      # weight elements read once per frame
    with _profiled("depth_frame", 2.0 * B * n_w, 2 * n_w + 4 * h_all.numel(), (B, t.dep_q, t.L)):
        _lib.check(fn(
            t.in_proj, t.out_proj, t.norm1, t.norm2, t.gate_in, t.gate_out, t.heads, t.head_bias, t.emb, t.emb_rows,
            _ptr(h_all), _ptr(tokens), _ptr(noise) if sampling else None, *lim, _ptr(ws), _ptr(t.status),
            B, t.E, t.H, t.Hd, t.card, t.dep_q, t.L, h_all.stride(0) if B > 1 else h_all.shape[1], tokens.stride(0) if B > 1 else tokens.shape[1],
            noise.stride(0) if (sampling and B > 1) else (noise.shape[1] if sampling else 0), int(top_k), int(sampling), float(temp), float(eps),
            _ctx(context), int(ring_cap) if ring_cap else t.dep_q, _stream()))


# ---- the temporal transformer of a batch-1 LM step (rst_temporal_decode_frame) ----------------------------------------------------------
# "auto": the persistent launch once the temporal rings hold at least TEMPORAL_FRAME_AUTO_POS steps.  Measured per frame (lm_b1, launch per
# op vs persistent, profiles/r06_temporal_persistent.txt): ring offset 0: 3.78 / 3.78 ms, 500: 3.90 / 3.95, 1000: 4.02 / 3.99, 2000: 4.08 /
# 4.08, 3000 (full): 4.20 / 4.14 -- the ring rows are part of its weight stream, so it gains where they are many.  True / False: always /
# never (tools/ab.py TEMPORAL_FRAME=True).
TEMPORAL_FRAME = "auto"
TEMPORAL_FRAME_AUTO_POS = 2048


def temporal_frame_wanted(host_pos: int) -> bool:
    """Whether a batch-1 temporal step at (host-side) position ``host_pos`` should take the persistent launch."""
    if TEMPORAL_FRAME == "auto":
        return host_pos >= TEMPORAL_FRAME_AUTO_POS
    return bool(TEMPORAL_FRAME)


TEMPORAL_FRAME_MAX_L = 40


def temporal_frame_supported(B: int, E: int, H: int, Hd: int, L: int, cap: int, kv_bf16: bool, device=None) -> bool:
    """Shapes ``rst_temporal_decode_frame`` serves -- the library's own answer (batch 1, E <= 4096, head dim 64 / 128, <= 40 layers, the
    LDS footprint, a workgroup per head, the occupancy query) -- on a device whose persistent launches have not been retired."""
    if not (TEMPORAL_FRAME and depth_frame_enabled(device) and B == 1 and 1 <= L <= TEMPORAL_FRAME_MAX_L and H >= 1 and E % max(H, 1) == 0):
        return False
    return _frame_grid("rst_temporal_frame_supported", _device_index(device), E, H, Hd, L, cap, int(kv_bf16)) > 0


class TemporalFrameTables:
    """Host arrays of device pointers of ``rst_temporal_decode_frame`` for one streaming session: the layers' weights (bf16), norm gains
    (fp32) and KV rings.  Keeps the tensors alive (a captured graph embeds the pointers)."""

    def __init__(self, layers: Sequence[dict], *, H: int, context: Optional[int], eps: float):
        """``layers``: dicts of device tensors ``in_proj [3E, E], out_proj [E, E], gate_in [2 Hd, E], gate_out [E, Hd]`` (bf16),
        ``norm1, norm2 [E]`` (fp32), ``k_cache, v_cache [1, H, cap, D]`` (bf16 or fp32)."""
        L = len(layers)
        keep = []

        def column(name, dtype):
            out = []
            for ly in layers:
                t = ly[name]
                if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype):
                    raise ValueError(f"rstnet_amd.ops: temporal-frame table {name!r} needs contiguous {dtype} device tensors")
                keep.append(t)
                out.append(t.data_ptr())
            return out
        E = layers[0]["out_proj"].shape[0]
        self.L, self.E, self.H, self.Hd = L, E, H, layers[0]["gate_out"].shape[1]
        kvd = layers[0]["k_cache"].dtype
        self.kv_bf16 = kvd == torch.bfloat16
        self.cap = layers[0]["k_cache"].shape[2]
        for ly in layers:
            assert tuple(ly["in_proj"].shape) == (3 * E, E) and tuple(ly["out_proj"].shape) == (E, E)
            assert tuple(ly["gate_in"].shape) == (2 * self.Hd, E) and tuple(ly["gate_out"].shape) == (E, self.Hd)
            assert tuple(ly["k_cache"].shape) == (1, H, self.cap, E // H) and ly["v_cache"].shape == ly["k_cache"].shape
        rows = [column("in_proj", torch.bfloat16), column("out_proj", torch.bfloat16), column("gate_in", torch.bfloat16),
                column("gate_out", torch.bfloat16), column("norm1", torch.float32), column("norm2", torch.float32), column("k_cache", kvd),
                column("v_cache", kvd)]
        # the [8][L] pointer table lives in device memory (addresses fit int64: the top bit of a device pointer is clear)
        self.dev_tables = torch.tensor(rows, dtype=torch.int64, device=layers[0]["in_proj"].device)
        self.context, self.eps = context, float(eps)
        self.status = new_persistent_status(layers[0]["in_proj"].device)
        self._keep = keep


@_on_tensor_device
def temporal_decode_frame(tables: "TemporalFrameTables", x: torch.Tensor, pos_dev: torch.Tensor, rope_table: Optional[torch.Tensor]) -> torch.Tensor:
    """x fp32 ``[1, E]`` -> ``[1, E]`` through every layer of ``tables`` (one new step at position ``*pos_dev``, appended to the rings);
    ``rope_table``: fp32 ``[D/2, 2]`` of `lm_rope_table` or None (no rotation)."""
    _chk(x, "x")
    _chk(pos_dev, "pos_dev", torch.int64)
    _shared_pos(pos_dev, "temporal_decode_frame")
    _chk(rope_table, "rope_table")
    t = tables
    assert x.shape == (1, t.E)
    y = torch.empty_like(x)
    ws = _frame_workspace("temporal_frame", x.device, (t.E, t.Hd, t.H))
    n_w = t.L * (4 * t.E * t.E + 3 * t.Hd * t.E)
    with _profiled("temporal_frame", 2.0 * n_w, 2 * n_w, (1, t.L, t.E)):
        _lib.check(_lib.lib().rst_temporal_decode_frame(
            _ptr(t.dev_tables), _ptr(x), _ptr(y), _ptr(pos_dev), _ptr(rope_table), _ptr(ws), _ptr(t.status), t.E, t.H, t.Hd, t.L, t.cap,
            _ctx(t.context), int(t.kv_bf16), t.eps, _stream()))
    return y


# ---- one streaming step of a Mimi transformer (rst_codec_transformer_frame) -------------------------------------------------------------
_ctr_status: dict = {}


def codec_transformer_frame_supported(B: int, T: int, E: int, H: int, F: int, L: int, cap: int, device=None) -> bool:
    """Shapes the persistent launch serves (else the launch-per-op layer loop runs) -- the library's own answer
    (rst_codec_transformer_supported: at most 4 rows and 4 new positions, <= 8 layers, head dim a multiple of 16 that divides 1024, a
    grid with rows for every workgroup and a workgroup per (stream, head), the occupancy query)."""
    if not (depth_frame_enabled(device) and B >= 1 and 1 <= T <= 4 and B * T <= 4 and H >= 1 and E % max(H, 1) == 0):
        return False
    return _frame_grid("rst_codec_transformer_supported", _device_index(device), B, T, E, H, F, L, cap) > 0


def codec_transformer_status(device) -> torch.Tensor:
    """The 4 device status words of the persistent codec-transformer launches of ``device`` (persist.h: [0] time-out codes of the step in
    flight, [1] steps repaired by the one-workgroup launch, [2] OR of the repaired codes)."""
    device = torch.device(device)
    st = _ctr_status.get(device)
    if st is None:
        st = _ctr_status[device] = new_persistent_status(device)
    return st


@_on_tensor_device
def codec_transformer_frame(x: torch.Tensor, layers: Sequence[dict], pos_dev: torch.Tensor, *, H: int, context: Optional[int], rope: bool,
                            max_period: float, eps: float) -> torch.Tensor:
    """x fp32 ``[B, T, E]`` (the new positions of every stream) -> ``[B, T, E]`` through all ``layers``: each a dict of fp32 device
    tensors ``in_proj [3E, E], out_proj [E, E], linear1 [F, E], linear2 [E, F], norm1_w/b, norm2_w/b [E], scale1/scale2 [E] or None,
    k_cache / v_cache [B, H, cap, D]`` (rings: the new steps are appended).  ``pos_dev``: int64 device scalar, position of x[:, 0]."""
    _chk(x, "x")
    _chk(pos_dev, "pos_dev", torch.int64)
    _shared_pos(pos_dev, "codec_transformer_frame")
    B, T, E = x.shape
    L = len(layers)
    F_ = layers[0]["linear1"].shape[0]
    cap = layers[0]["k_cache"].shape[2]
    for ly in layers:
        for name in ("in_proj", "out_proj", "linear1", "linear2", "norm1_w", "norm1_b", "norm2_w", "norm2_b", "k_cache", "v_cache"):
            _chk(ly[name], name)
        _chk(ly.get("scale1"), "scale1"); _chk(ly.get("scale2"), "scale2")

    def table(name):
        return (C.c_void_p * L)(*[_ptr(ly.get(name)) for ly in layers])
    has_scale = layers[0].get("scale1") is not None
    y = torch.empty_like(x)
    ws = _frame_workspace("codec_transformer", x.device, (B * T, E, F_))
    D = E // H
    _lib.check(_lib.lib().rst_codec_transformer_frame(
        table("in_proj"), table("out_proj"), table("linear1"), table("linear2"), table("norm1_w"), table("norm1_b"), table("norm2_w"),
        table("norm2_b"), table("scale1") if has_scale else None, table("scale2") if has_scale else None, table("k_cache"), table("v_cache"),
        _ptr(x), _ptr(y), _ptr(pos_dev), _ptr(ws), _ptr(codec_transformer_status(x.device)), B, T, E, H, F_, L, cap,
        _ctx(context), int(rope), rope_coef(max_period, D), float(eps), _stream()))
    return y
