"""Launch recording, route labels and fp64 references for the many-stream codec step tests (tests/test_codec_streams_gpu.py).

`record_frame` runs one eager streamed Mimi frame (encode and decode) and writes down every GEMM-like call the codec makes through
`ops` -- with all the sizes and switches that pick a kernel -- so that the tests can replay each call with random operands against
an fp64 reference, and `route_of` names the kernel configuration each call reaches (the launcher's own rules: gemm_win.hip
gw_tile_cfg / rst_launch_gemm_win, ops._few_rows, skinny_f32.hip)."""
import contextlib

import torch
import torch.nn.functional as F

from rstnet_amd import _lib, ops
from rstnet_amd.codec import functional as RF

U = 2.0 ** -24
FRAME = 1920


def unpack_f32(xp: torch.Tensor, K: int) -> torch.Tensor:
    """Packed fp32 operand of the few-row GEMM (rst_common.h f32_packed_index: [tile of 32 rows][Kp / 8][k % 2][row % 32][k % 8 / 2])
    -> row-major ``[rows, Kp]``."""
    Kp = (K + 7) // 8 * 8
    return xp.reshape(-1, Kp // 8, 2, 32, 4).permute(0, 3, 1, 4, 2).reshape(-1, Kp)


def pack_rows(x: torch.Tensor) -> torch.Tensor:
    """Row-major ``[M, K]`` (M <= 128) -> the packed operand, by the library's own plain packing launch (no window, no history)."""
    M, K = x.shape
    xp = torch.empty(32 if M <= 32 else (64 if M <= 64 else 128), (K + 7) // 8 * 8, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().rst_skinny_f32_pack_win(x.data_ptr(), None, xp.data_ptr(), 1, M, M, K, K, 1, 0, 0, M * K, 0,
                                                 torch.cuda.current_stream().cuda_stream))
    return xp


# ---------------------------------------------------------------------------------------------------------------- recording

@contextlib.contextmanager
def recording(launches: list):
    """Inside the block every ops.gemm_win / ops.linear / ops.attention_step / ops.seanet_resblock call appends a record."""
    saved = {n: getattr(ops, n) for n in ("gemm_win", "linear", "attention_step", "seanet_resblock")}
    saved_tr = RF.convtr1d
    convtr = []

    def gemm_win(x, w, **kw):
        hist = kw.get("hist")
        launches.append(dict(kind="gemm_win", B=kw["B"], T_in=kw["T_in"], T_out=kw["T_out"], C=kw["C_"], S=kw["S"], P=kw["P"], N=kw["N"],
                             K=w.shape[1], hist=hist is not None, bias=kw.get("bias") is not None, res=kw.get("res") is not None,
                             scale=kw.get("scale") is not None, pad_mode=kw.get("pad_mode", ops.PAD_ZERO),
                             act_in=kw.get("act_in", ops.ACT_NONE), act_out=kw.get("act_out", ops.ACT_NONE),
                             convtr=convtr[-1] if convtr else None))
        return saved["gemm_win"](x, w, **kw)

    def convtr1d(x, w, bias, *, kernel, stride, **kw):
        convtr.append((kernel, stride))
        try:
            return saved_tr(x, w, bias, kernel=kernel, stride=stride, **kw)
        finally:
            convtr.pop()

    def linear(x, w, bias=None, **kw):
        packed_in = isinstance(x, ops.PackedRows)
        K = x.shape[-1]
        M = 1
        for d in x.shape[:-1]:
            M *= d
        launches.append(dict(kind="linear", M=M, N=w.shape[0], K=K, packed_in=packed_in, out_packed=bool(kw.get("out_packed", False)),
                             ln=kw.get("ln") is not None, bias=bias is not None, res=kw.get("res") is not None,
                             scale=kw.get("scale") is not None, act_out=kw.get("act_out", ops.ACT_NONE)))
        return saved["linear"](x, w, bias, **kw)

    def attention_step(qkv, H, k, v, pos_dev, **kw):
        launches.append(dict(kind="attention_step", B=qkv.shape[0], T=qkv.shape[1], H=H, D=qkv.shape[2] // (3 * H), cap=k.shape[2],
                             context=kw.get("context"), rope=kw.get("rope", True), out_packed=bool(kw.get("out_packed", False))))
        return saved["attention_step"](qkv, H, k, v, pos_dev, **kw)

    def seanet_resblock(x, *a, **kw):
        launches.append(dict(kind="resblock", B=x.shape[0], T=x.shape[1], C=x.shape[2], hist=kw.get("hist") is not None))
        return saved["seanet_resblock"](x, *a, **kw)

    for n, f in (("gemm_win", gemm_win), ("linear", linear), ("attention_step", attention_step), ("seanet_resblock", seanet_resblock)):
        setattr(ops, n, f)
    RF.convtr1d = convtr1d
    try:
        yield launches
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
        RF.convtr1d = saved_tr


def record_frame(model, S: int, card: int, seed: int = 0):
    """Two eager warm-up frames of S streams (every history reaches its steady length), then the third eager frame recorded:
    returns (launches of encode, launches of decode, ops.PROFILE rows of encode + decode)."""
    dev = next(model.parameters()).device
    g = torch.Generator().manual_seed(seed)
    audio = 0.1 * torch.randn(S, 1, 3 * FRAME, generator=g)
    codes = torch.randint(0, card, (S, 8, 3), generator=g)
    enc, dec = [], []
    with model.streaming(S), torch.no_grad():
        for f in range(3):
            a = audio[:, :, f * FRAME:(f + 1) * FRAME].contiguous().to(dev)
            c = codes[:, :, f:f + 1].contiguous().to(dev)
            if f < 2:
                model.quantizer.encode_nlc(model.encode_latent(a))
                model._decode(c)
                continue
            torch.cuda.synchronize()
            ops.PROFILE = []
            try:
                with recording(enc):
                    model.quantizer.encode_nlc(model.encode_latent(a))
                with recording(dec):
                    model._decode(c)
                torch.cuda.synchronize()
                prof = [(r[0], tuple(r[5])) for r in ops.PROFILE]
            finally:
                ops.PROFILE = None
    return enc, dec, prof


# ---------------------------------------------------------------------------------------------------------------- routes

def cu_count() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _gemm_win_route(M: int, N: int, K: int, x_aligned: bool = True) -> str:
    """The f32 gemm_win configuration rst_launch_gemm_win picks (split-K from the library's plan)."""
    split = int(_lib.lib().rst_gemm_win_split_plan(M, N, K)) if M <= 4096 else 1
    if N > 64 and M > 4096:
        tiles = -(-M // 128) * -(-N // 128)
        if tiles < cu_count():
            return f"gemm_win 128x128 under-filled -> 32x128 ({tiles} tiles)"
        return f"gemm_win tile-streaming 128x128 KB{16 if tiles >= 768 else 32}" if x_aligned else "gemm_win 128x128"
    tile = "32x128" if N > 64 else ("128x64" if N > 32 else "256x32")
    return f"gemm_win {tile}" + (f" split-K {split}" if split > 1 else "")


def _skinny_split(M: int, N: int, K: int) -> int:
    return int(_lib.lib().rst_skinny_f32_split_plan(M, N, K))


def route_of(rec: dict) -> str:
    """Kernel configuration a recorded call reaches (ops.gemm_win / ops.linear / ops.attention_step route rules)."""
    if rec["kind"] == "attention_step":
        return "attention_step packed" if rec["out_packed"] else "attention_step"
    if rec["kind"] == "resblock":
        return "resblock"
    if rec["kind"] == "gemm_win":
        M, N, K = rec["B"] * rec["T_out"], rec["N"], rec["K"]
        if ops._few_rows(M, N, K):
            plain = not rec["hist"] and rec["S"] == 1 and rec["P"] == 0 and rec["T_in"] == rec["T_out"] and rec["C"] == K and rec["act_in"] == 0
            s = _skinny_split(M, N, K)
            how = "linear_few_rows" if plain and K % 8 == 0 else "pack_win"
            return f"skinny_f32 {how}" + (f" split-K {s}" if s > 1 else "")
        if _b3(rec):
            return "gemm_win_b3 three-plane bf16 128x%d" % (256 if N >= 256 else 128)
        return _gemm_win_route(M, N, K)
    M, N, K = rec["M"], rec["N"], rec["K"]
    if rec["packed_in"] or rec["out_packed"]:
        s = _skinny_split(M, N, K)
        how = "packed in" if rec["packed_in"] else ("pack_ln" if rec["ln"] else "linear_few_rows")
        return f"skinny_f32 {how}" + (" -> packed out" if rec["out_packed"] else "") + (f" split-K {s}" if s > 1 else "")
    if 1 <= M <= 4 and K % 8 == 0 and K * M <= 32768 and rec["act_out"] in (ops.ACT_NONE, ops.ACT_GELU):
        return "gemv_f32"
    if ops._few_rows(M, N, K):
        s = _skinny_split(M, N, K)
        how = "pack_ln" if rec["ln"] and K % 4 == 0 else ("linear_few_rows" if K % 8 == 0 else "pack_win")
        return f"skinny_f32 {how}" + (f" split-K {s}" if s > 1 else "")
    split = int(_lib.lib().rst_gemm_win_split_plan(M, N, K)) if M <= 4096 else 1
    return _gemm_win_route(M, N, K) if split > 1 else "linear_f32"


def _b3(rec: dict) -> bool:
    """ops.gemm_win's choice of the three-plane kernel for a recorded call (ops._b3_route on 16-byte-aligned operands)."""
    M, N, K = rec["B"] * rec["T_out"], rec["N"], rec["K"]
    split = int(_lib.lib().rst_gemm_win_split_plan(M, N, K)) if M <= 4096 else 1
    return (split <= 1 and ops._b3_shape(M, N, K) and
            ops._b3_supported(rec["B"], rec["T_in"], rec["T_out"], rec["C"], K, N, rec["S"], rec["P"], rec["pad_mode"], rec["T_in"] * rec["C"],
                              rec["hist"]))


def key_of(rec: dict) -> tuple:
    """(profile name, M, N, K) under which ops.PROFILE lists the call (None: a route that writes no profile row)."""
    if rec["kind"] == "gemm_win":
        M, N, K = rec["B"] * rec["T_out"], rec["N"], rec["K"]
        return ("gemm_skinny_f32" if ops._few_rows(M, N, K) else "gemm_win_b3" if _b3(rec) else "gemm_win", M, N, K)
    if rec["kind"] == "linear":
        r = route_of(rec)
        if r == "gemv_f32":
            return None
        return ("gemm_skinny_f32" if r.startswith("skinny") else "gemm_win", rec["M"], rec["N"], rec["K"])
    if rec["kind"] == "resblock":
        return None
    return None


# ---------------------------------------------------------------------------------------------------------------- fp64 references

def epilogue64(acc, mag, bias, res, scale, act_out):
    """gemm_win's epilogue (bias -> GELU? -> res + scale * . -> ELU?) on fp64 ``acc`` and the magnitude its rounding errors scale with:
    returns (reference, per-element bound magnitude M, so that a backward-stable result has |y - ref| <= c * 2^-24 * M)."""
    y = acc + (bias if bias is not None else 0.0)
    m = mag + (bias.abs() if bias is not None else 0.0)
    if act_out == ops.ACT_GELU:
        y, m = F.gelu(y), 1.13 * m + y.abs()              # |GELU'| <= 1.13; erf's own rounding relative to the result
    if res is not None:
        s = scale if scale is not None else 1.0
        y = res + s * y
        m = (s.abs() if scale is not None else 1.0) * m + res.abs() + y.abs()
    if act_out == ops.ACT_ELU_OUT:
        y = F.elu(y)
        m = m + y.abs()                                   # |ELU'| <= 1
    return y, m


def window_rows(seq: torch.Tensor, taps: int, stride: int, T_out: int) -> torch.Tensor:
    """``seq [B, L, C]`` -> the windowed A operand ``[B, T_out, taps * C]`` (index tap * C + c: pack_conv_weight's order)."""
    B, L, C = seq.shape
    w = seq.unfold(1, taps, stride)[:, :T_out]            # [B, T_out, C, taps]
    return w.permute(0, 1, 3, 2).reshape(B, T_out, taps * C)


def layernorm64(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    """fp64 LayerNorm and the per-element magnitude of its rounding errors (|x_hat * gamma| + |beta|)."""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    xh = (x - mu) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
    return xh * gamma.double() + beta.double(), (xh * gamma.double()).abs() + beta.double().abs()
