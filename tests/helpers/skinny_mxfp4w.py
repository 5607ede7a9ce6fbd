"""CPU restatement of the operand of the weight-only MXFP4 skinny GEMM (csrc/lm_skinny.hip: skinny_pack_weight_mxfp4w_kernel,
gemm_skinny_kernel<NB, CT, false, true>) and the weights its tests share.  Nothing here needs a GPU.

Packed codes ``qp``: the stored ``q [N, K/2]`` code bytes of ``ops.quantize_blocks_mxfp4`` (two e2m1 codes per byte, even k in the low
nibble) in the order of the fp8 operand at half the bytes -- [tile of 32 rows][K/32][64 lanes = 32 * ((k / 8) % 2) + row % 32][8 B =
the 4 code bytes of the lane's 8 k of step 2p | of step 2p+1]; byte offset of (packed row r, k), nibble k % 2:

    ((((r / 32) * (K / 32) + k / 32) * 64) + ((k / 8) % 2) * 32 + r % 32) * 8 + ((k / 16) % 2) * 4 + (k % 8) / 2

A pair of steps is one 32-k scale block, so the 8 bytes a lane loads need exactly one scale byte.  Packed scales ``sp``: uint8
``[tile][K/32][32 rows]``, i.e. byte ``((r / 32) * (K / 32) + k / 32) * 32 + r % 32`` (no regrouping).  Packed row r holds source row
``src_rows(N, interleave)[r]`` as in helpers.skinny_fp8w (gated layers: tile t = u rows 16t .. 16t+15, then the matching v rows), codes
and scale bytes alike.  Rows N .. ceil(N/32)*32 - 1 are pad: zero codes, scale byte 127 (= 2^0).  Nothing depends on the batch size."""
import numpy as np
import torch

from tests.helpers import skinny_fp8w as S8
from tests.helpers.gemv_bounds import mixed_rows

rows32 = S8.rows32
src_rows = S8.src_rows
PAD_SCALE = 127


def code_offsets(N: int, K: int) -> np.ndarray:
    """Byte offset of the code pair (k, k + 1) of every (packed row, k / 2): int64 ``[rows32(N), K / 2]``."""
    assert K % 32 == 0
    r, k = np.meshgrid(np.arange(rows32(N)), np.arange(0, K, 2), indexing="ij")
    return ((((r // 32) * (K // 32) + k // 32) * 64) + ((k // 8) % 2) * 32 + r % 32) * 8 + ((k // 16) % 2) * 4 + (k % 8) // 2


def scale_offsets(N: int, K: int) -> np.ndarray:
    """Byte offset in ``sp`` of the scale byte of every (packed row, block of 32 k): int64 ``[rows32(N), K / 32]``."""
    assert K % 32 == 0
    r, blk = np.meshgrid(np.arange(rows32(N)), np.arange(K // 32), indexing="ij")
    return ((r // 32) * (K // 32) + blk) * 32 + r % 32


def pack_weight_ref(q: torch.Tensor, scale: torch.Tensor, interleave: bool = False):
    """(q uint8 [N, K/2], scale uint8 [N, K/32]) on the CPU -> (qp uint8 [rows32 * K/2], sp uint8 [rows32 * K/32]) in device byte order."""
    N, K = q.shape[0], 2 * q.shape[1]
    assert scale.shape == (N, K // 32)
    src = src_rows(N, interleave)
    live = src >= 0
    rows = np.zeros((rows32(N), K // 2), np.uint8)
    rows[live] = q.numpy()[src[live]]
    srows = np.full((rows32(N), K // 32), PAD_SCALE, np.uint8)
    srows[live] = scale.numpy()[src[live]]
    qp = np.zeros(rows32(N) * (K // 2), np.uint8)
    qp[code_offsets(N, K).ravel()] = rows.ravel()
    sp = np.zeros(rows32(N) * (K // 32), np.uint8)
    sp[scale_offsets(N, K).ravel()] = srows.ravel()
    return torch.from_numpy(qp), torch.from_numpy(sp)


def unpack_ref(qp: torch.Tensor, sp: torch.Tensor, N: int, K: int):
    """The inverse read, as the kernel's lanes perform it: packed row r, pair p -> the lane's 8 bytes (both halves of the block) and the
    ONE scale byte that goes with them.  Returns (codes uint8 [rows32, K/2] in k order, scale bytes uint8 [rows32, K/32])."""
    return (torch.from_numpy(qp.numpy()[code_offsets(N, K)]), torch.from_numpy(sp.numpy()[scale_offsets(N, K)]))


def block_weights(N: int, K: int, g: torch.Generator) -> torch.Tensor:
    """bf16 ``[N, K]``: randn times 2^e with e drawn independently per block of 32 k in [-15, 15] -- a block decoded with a neighbour's
    scale is off by a factor of two or more almost everywhere -- and row 1 all zero."""
    e = torch.randint(-15, 16, (N, K // 32), generator=g)
    w = (torch.randn(N, K // 32, 32, generator=g) * torch.exp2(e.double()).float()[:, :, None]).view(N, K)
    w[1] = 0
    return w.bfloat16()


def exhaustive_codes(K: int = 32, block: int = 0):
    """Hand-built ``(q [244, K/2], scale [244, K/32])``: row i carries scale byte 2 + i (2 .. 245: every exponent the quantiser can emit)
    in block ``block`` and holds all 16 codes twice there (k = 0..15 -> codes 0..15, k = 16..31 again); every other block holds code 2
    (= 1.0) throughout under the scale byte 127 - 9 * ((i % 5) + 1), never the row's own, so a neighbour's scale shows."""
    N = 244
    codes = torch.full((N, K), 2, dtype=torch.int64)
    codes[:, 32 * block:32 * block + 32] = torch.arange(32) % 16
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    scale = (127 - 9 * ((torch.arange(N) % 5) + 1))[:, None].repeat(1, K // 32)
    scale[:, block] = 2 + torch.arange(N)
    return q.contiguous(), scale.to(torch.uint8).contiguous()


# (B, N, K, prologue, res, bias) of the fp64 bound test
BOUND_CASES = [(3, 1001, 1024, 0, False, False),        # ragged N, one batch tile
               (4, 33, 4096, 1, False, False),          # a second column tile with a single live row
               (5, 96, 8192, 0, True, True),            # K split below 33 rows
               (31, 9001, 288, 2, False, False),        # 9 pairs, 18 steps over 8 waves: waves start on odd steps
               (32, 17001, 512, 1, False, False),       # more column tiles than CUs
               (33, 4099, 4096, 1, False, False),       # two batch tiles, split at K >= 4096
               (64, 4096, 8192, 2, True, False)]        # two batch tiles with a deep split


def bound_inputs(B, N, K, mode, res, bias):
    """The CPU operands of a bound case: (x, alpha, res or None, bias or None, bf16 weights to quantise)."""
    g = torch.Generator().manual_seed(B * 1000 + N + K)
    x = mixed_rows(B, 2 * K if mode == 2 else K, g)
    alpha = 1 + 0.1 * torch.randn(K, generator=g)
    r = torch.randn(B, N, generator=g) if res else None
    b = torch.randn(N, generator=g) if bias else None
    return x, alpha, r, b, block_weights(N, K, g)
