"""CPU restatement of the operand of the weight-only fp8 skinny GEMM (csrc/lm_skinny.hip: skinny_pack_weight_fp8w_kernel,
gemm_skinny_kernel<NB, CT, true>) and the error bound of the product.  Nothing here needs a GPU.

Packed weight: the stored ``q [N, K]`` e4m3fn bytes of ``ops.quantize_rows_fp8`` in the order the bf16 MFMA consumes them, two 16-k
steps per 16-byte lane load -- byte offset of (packed row r, k):

    ((((r / 32) * (K / 32) + k / 32) * 64) + ((k / 8) % 2) * 32 + r % 32) * 16 + ((k / 16) % 2) * 8 + k % 8

(``helpers.lm_operands.fp8_packed_index``).  Packed row r holds source row ``src_rows(N, interleave)[r]``: r itself, or with
``interleave`` (gated layers, ``q = [Q_u ; Q_v]``, N % 32 == 0) tile t = r / 32 holds u rows 16t .. 16t+15 and then the matching v
rows N/2 + 16t .. N/2 + 16t+15.  Rows N .. ceil(N/32)*32 - 1 are pad: zero bytes, scale 0.  The scales travel in packed row order."""
import numpy as np
import torch  # noqa: F401

from tests.helpers import lm_fp8w as Q
from tests.helpers import lm_operands as O

U = Q.U
C_PROLOGUE = Q.C_PROLOGUE


def rows32(N: int) -> int:
    return (N + 31) // 32 * 32


def src_rows(N: int, interleave: bool = False) -> np.ndarray:
    """Source row of every packed row, -1 for a pad row."""
    r = np.arange(rows32(N), dtype=np.int64)
    if interleave:
        assert N % 32 == 0
        return np.where(r % 32 < 16, 0, N // 2) + (r // 32) * 16 + r % 16
    return np.where(r < N, r, -1)


def packed_offsets(N: int, K: int) -> np.ndarray:
    """Byte offset of every (packed row, k): int64 ``[rows32(N), K]``."""
    assert K % 32 == 0
    r, k = np.meshgrid(np.arange(rows32(N)), np.arange(K), indexing="ij")
    return O.fp8_packed_index(r, k, K)


def pack_weight_ref(q: torch.Tensor, scale: torch.Tensor, interleave: bool = False):
    """(q uint8 [N, K], scale fp32 [N]) on the CPU -> (qp uint8 [rows32 * K] in device byte order, sp fp32 [rows32])."""
    N, K = q.shape
    src = src_rows(N, interleave)
    live = src >= 0
    rows = np.zeros((rows32(N), K), np.uint8)
    rows[live] = q.numpy()[src[live]]
    qp = np.zeros(rows32(N) * K, np.uint8)
    qp[packed_offsets(N, K).ravel()] = rows.ravel()
    sp = np.zeros(rows32(N), np.float32)
    sp[live] = scale.numpy()[src[live]]
    return torch.from_numpy(qp), torch.from_numpy(sp)


def acc(K: int) -> float:
    """The fp32 accumulation bound of one output of the skinny MFMA GEMM relative to sum_k |x_k| |w_k|, as
    tests/test_lm_operands_gpu.py::_acc states it: a wave's sequential chain covers K/8 of the contraction in 16-k steps, hi and lo one
    accumulation each -> K/64 roundings, plus at most 32 for the instruction's own 16-term sums, the wave and split reductions, the
    per-row scale and the bias."""
    return (K / 64 + 32) * U


def bound(K: int, prologue: int) -> float:
    """Backward-error bound of ``ops.gemm_skinny_fp8w`` on ``(q, scale)`` against fp64 ``P(x) @ dequant(q, scale).T``, relative to
    ``sum_k |P(x)_k| |w_k|`` (+ |bias| + |res|): the bf16 packed route's.  The decode e4m3 -> bf16 is exact (4 significant bits into 8)
    and so is the power-of-two row scale on the fp32 accumulator (away from underflow), so the only errors are the hi / lo split of the
    activations (SPLIT_BOUND = 2^-16), the fp32 accumulation (``acc``) and, with a prologue, its fp32 evaluation (C_PROLOGUE * 2^-24)."""
    return O.SPLIT_BOUND + acc(K) + (C_PROLOGUE * U if prologue else 0.0)


def underflow_floor(split: int) -> float:
    """Absolute term next to ``bound`` for outputs below fp32's normal range (|y| < 2^-126; the tests' row of scale < 2^-100 against
    activation rows of 2^-20, squared by the SiLU gate, lands there): the output format itself resolves 2^-149 there, whatever computes
    it.  A partial tile times the row scale may round to that grid, half a unit each, once per wave (8) and K split; sums of subnormal
    numbers are exact.  Normal results are not affected: the term is below 2^-23 of the smallest of them."""
    return 8 * max(split, 1) * 2.0 ** -150
