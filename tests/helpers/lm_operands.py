"""CPU restatements of the LM skinny GEMM's operand formats (csrc/lm_common.h, csrc/lm_skinny.hip), for the operand tests.

- the two MFMA-ordered layouts: bf16 ``[tile of 32 rows][K/16][64 lanes][8]`` (packed_index) and fp8 ``[tile][K/32][64][16 B]``
  (fp8_packed_index), as index formulas and as the reshapes that decode a whole buffer;
- split_hi_lo: bit-exact emulation of split_hi_lo8 (hi = the fp32 value truncated to bf16, lo = the residual x - hi rounded
  half-up, i.e. half away from zero in magnitude, by adding 0x8000 to its bits);
- bf16_rne: fp32 -> bf16 round to nearest even, NaN kept NaN (the ring appends, bf16_rne of lm_common.h).

All bit patterns are numpy uint16 / uint32 arrays; nothing here needs a GPU."""
import numpy as np
import torch

# |x - (hi + lo)| <= SPLIT_BOUND * |x| (+ half the smallest bf16 subnormal when the residual is subnormal): the truncated hi leaves
# |r| < ulp(hi) <= 2^-7 |x|, so r's exponent is at least 8 below x's; rounding r to bf16 (8 significant bits) costs at most half an
# ulp of r, 2^(e_r - 8) <= 2^(e_x - 16) <= 2^-16 |x|.  Attained: x = 1 + 2^-8 + 2^-16 (0x3F808080) leaves the tie r = 2^-8 + 2^-16,
# which lo rounds up to 2^-8 + 2^-15: error 2^-16.  (x = 0x3F80FFFF leaves r = 2^-7 - 2^-23, which carries into lo = 2^-7.)
SPLIT_BOUND = 2.0 ** -16
BF16_SUBNORMAL_HALF = 2.0 ** -134


def packed_index(row, k, K: int):
    """Element offset of (row, k) in one plane of the bf16 layout (lm_common.h packed_index)."""
    row, k = np.asarray(row, np.int64), np.asarray(k, np.int64)
    return ((((row >> 5) * (K >> 4) + (k >> 4)) * 64) + ((k >> 3) & 1) * 32 + (row & 31)) * 8 + (k & 7)


def fp8_packed_index(row, k, K: int):
    """Byte offset of (row, k) in the fp8 layout (lm_skinny.hip fp8_packed_index)."""
    row, k = np.asarray(row, np.int64), np.asarray(k, np.int64)
    return ((((row >> 5) * (K >> 5) + (k >> 5)) * 64) + ((k >> 3) & 1) * 32 + (row & 31)) * 16 + ((k >> 4) & 1) * 8 + (k & 7)


def decode_packed(plane: torch.Tensor, K: int) -> torch.Tensor:
    """One packed bf16 plane (any shape, ``rows32 * K`` 16-bit elements) -> ``[rows32, K]`` in row-major order, same dtype.
    [tile][k / 16][k / 8 % 2][row % 32][k % 8] -> [tile][row % 32][k / 16][k / 8 % 2][k % 8]."""
    t = plane.reshape(-1, K // 16, 2, 32, 8)
    return t.permute(0, 3, 1, 2, 4).reshape(-1, K)


def decode_fp8(buf: torch.Tensor, K: int) -> torch.Tensor:
    """The fp8 operand (``rows32 * K`` bytes) -> ``[rows32, K]`` bytes in row-major order.
    [tile][k / 32][k / 8 % 2][row % 32][k / 16 % 2][k % 8] -> [tile][row % 32][k / 32][k / 16 % 2][k / 8 % 2][k % 8]."""
    t = buf.reshape(-1, K // 32, 2, 32, 2, 8)
    return t.permute(0, 3, 1, 4, 2, 5).reshape(-1, K)


def bits16(t: torch.Tensor) -> np.ndarray:
    """bf16 / int16 tensor -> numpy uint16 bit patterns."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def f32_bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bf16_to_f32(b) -> np.ndarray:
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def is_nan16(b) -> np.ndarray:
    return (np.asarray(b, np.uint16) & 0x7FFF) > 0x7F80


def split_hi_lo(x) -> tuple:
    """Bit-exact split_hi_lo8 of fp32 values (gradual underflow, the GPU's fp32 mode): -> (hi, lo) uint16.  For NaN residuals (x = NaN
    or +-Inf: Inf - Inf) the payload is the platform's; compare those with ``is_nan16`` only."""
    u = f32_bits(x)
    hi = (u >> 16).astype(np.uint16)
    with np.errstate(invalid="ignore", over="ignore"):
        r = u.view(np.float32) - (u & np.uint32(0xFFFF0000)).view(np.float32)       # exact: hi is a prefix of x
    lo = ((r.view(np.uint32) + np.uint32(0x8000)) >> 16).astype(np.uint16)           # 32-bit add: wraps like the device's
    return hi, lo


def bf16_rne(x) -> np.ndarray:
    """fp32 -> bf16 round to nearest, ties to even (overflow to +-Inf); NaN -> NaN with the quiet bit set (sign and top payload kept)."""
    u = f32_bits(x)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)
    return np.where(nan, ((u >> 16) | np.uint32(0x40)).astype(np.uint16), r)


def bf16_boundary_distance_ulps(x) -> np.ndarray:
    """Distance of fp32 values to the nearest bf16 rounding boundary (the midpoint between two bf16 neighbours), in fp32 ulps:
    the low 16 bits of the pattern against 0x8000."""
    return np.abs((f32_bits(x) & np.uint32(0xFFFF)).astype(np.int64) - 0x8000)


def same_bits16(a, b) -> np.ndarray:
    """Element-wise: equal bit patterns, or both NaN."""
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    return (a == b) | (is_nan16(a) & is_nan16(b))


def fp8_quant_ref(t: torch.Tensor) -> tuple:
    """The per-row e4m3 quantiser the fp8 path restates: scale = amax / 448 in fp32 (1 for an all-zero row), bytes = RNE of t / scale.
    t fp32 [rows, K] -> (bytes uint8 [rows, K], scale fp32 [rows])."""
    t = t.float()
    amax = t.abs().amax(dim=1)
    sc = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    q = (t / sc[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, sc


def fp8_to_f64(q: torch.Tensor) -> torch.Tensor:
    return q.view(torch.float8_e4m3fn).double()
