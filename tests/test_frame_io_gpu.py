"""The packed frame records on the GPU (csrc/frame_io.hip): ``ops.frame_egress`` against ``slots.egress_reference`` -- which is
``PcmFramer.encode`` per row --, the whole ``[B, REC]`` buffer byte for byte, headers and padding included; ``ops.frame_ingress`` against
the numpy formula of ``PcmFramer.frames``, bit for bit.

Shapes: three rows; F = 5 (tail lanes only), 882 (rows of the fp32 side off a 16-byte boundary, a record stride that needs the rounding)
and 1920 (the real frame, more than one workgroup per row on the egress); the rows' formats {f32, s16, free} in every rotation; frame
counters {0, max_delay, max_delay + 1} for max_delay in {0, 1} in every rotation against the formats.  Both launches write into a buffer
with one row more than the batch, which must keep its fill."""
import numpy as np
import pytest
import torch

from rstnet_amd import ops
from rstnet_amd import slots as SL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
FORMATS = [SL.FMT_F32, SL.FMT_S16, SL.FMT_FREE]
SIZES = [5, 882, 1920]


def _rot(xs, r):
    return xs[r:] + xs[:r]


def _specials() -> np.ndarray:
    """Where the s16 encoding can go wrong: the clamp's ends and their neighbours, zeros, a denormal-range value, infinities, and for
    several k the floats on either side of k / 32767 (truncation toward zero decides between k - 1 and k)."""
    one = np.float32(1.0)
    v = [one, -one, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(-2)),
         np.nextafter(-one, np.float32(0)), np.float32(0.0), np.float32(-0.0), np.float32(1e-30), np.float32(-1e-30),
         np.float32(np.inf), np.float32(-np.inf)]
    for k in (1, 2, 3, 100, 12345, 16383, 16384, 32766, 32767):
        for sign in (1, -1):
            x = np.float32(sign * k) / np.float32(32767.0)
            v += [x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-2))]
    return np.array(v, dtype=np.float32)


def _wav(F: int, window: int, seed: int) -> np.ndarray:
    """fp32 [B, 1, F]: a seeded random fill (some of it beyond +-1) with the special values laid over its start, from ``window`` on and at
    another phase in every row."""
    rng = np.random.default_rng(seed)
    wav = (0.6 * rng.standard_normal((B, 1, F))).astype(np.float32)
    sp = _specials()
    n = min(F, len(sp))
    for b in range(B):
        wav[b, 0, :n] = sp[(np.arange(n) + window + 5 * b) % len(sp)]
    return wav


def _egress(wav: np.ndarray, tokens: np.ndarray, offsets, max_delay: int, fmt, F: int) -> np.ndarray:
    REC = SL.record_stride(F)
    guard = torch.full((B + 1, REC), 0xA5, dtype=torch.uint8, device=DEV)
    out = ops.frame_egress(torch.from_numpy(wav).to(DEV), torch.from_numpy(tokens).to(DEV), torch.tensor(offsets, dtype=torch.long, device=DEV),
                           max_delay, torch.tensor(fmt, dtype=torch.int32, device=DEV), guard[:B])
    assert out.data_ptr() == guard.data_ptr()
    got = guard.cpu().numpy()
    assert (got[B] == 0xA5).all(), "the egress wrote past the batch"
    return got[:B]


@pytest.mark.parametrize("rotation", [0, 1, 2])
@pytest.mark.parametrize("F", SIZES)
def test_egress_equals_the_reference_byte_for_byte(F, rotation):
    fmt = _rot(FORMATS, rotation)
    n_sp = len(_specials())
    windows = list(range(0, n_sp, F)) if F < n_sp else [0]          # F = 5: every special value passes through the five tail lanes
    rng = np.random.default_rng(100 * F + rotation)
    tokens = rng.integers(0, 32000, (B, 9)).astype(np.int64)
    for window in windows:
        wav = _wav(F, window, seed=F + window)
        for max_delay in (0, 1):
            for r in range(3):
                offsets = _rot([0, max_delay, max_delay + 1], r)
                want = SL.egress_reference(wav, tokens, offsets, max_delay, fmt, F)
                got = _egress(wav, tokens, offsets, max_delay, fmt, F)
                assert got.shape == want.shape == (B, SL.record_stride(F))
                if not np.array_equal(got, want):
                    bad = np.argwhere(got != want)
                    raise AssertionError(f"F={F} fmt={fmt} offsets={offsets} max_delay={max_delay}: {len(bad)} bytes differ, first at {bad[0].tolist()}")
    # the cases are not vacuous: a valid s16 row and a valid f32 row occurred
    want = SL.egress_reference(wav, tokens, [9, 9, 9], 1, fmt, F)
    assert sorted(want[:, :4].view("<i4")[:, 0].tolist()) == [0, 1, 1]


@pytest.mark.parametrize("F", SIZES)
def test_egress_nan_encodes_as_zero(F):
    wav = _wav(F, 0, seed=7)
    for b in range(B):
        wav[b, 0, [0, F // 2, F - 1]] = np.float32(np.nan)           # head, body and tail lanes
    wav[1, 0, 1] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), dtype=np.float32)[0]      # a negative NaN with a payload
    tokens = np.arange(B * 9, dtype=np.int64).reshape(B, 9)
    fmt = [SL.FMT_S16, SL.FMT_S16, SL.FMT_F32]
    got = _egress(wav, tokens, [5, 5, 5], 1, fmt, F)
    want = SL.egress_reference(wav, tokens, [5, 5, 5], 1, fmt, F)
    assert np.array_equal(got, want)
    for b in (0, 1):
        s16 = np.frombuffer(got[b, 16:16 + 2 * F].tobytes(), dtype="<i2")
        assert s16[0] == 0 and s16[F // 2] == 0 and s16[F - 1] == 0 and (b == 0 or s16[1] == 0)
    assert got[2, 16:16 + 4 * F].tobytes() == wav[2, 0].tobytes()     # an f32 row carries the NaN's bits unchanged


def _ingress(staged: np.ndarray, fmt, F: int, rows: int = B) -> np.ndarray:
    guard = torch.full((rows + 1, 1, F), float("nan"), device=DEV)
    out = ops.frame_ingress(torch.from_numpy(staged).to(DEV), torch.tensor(fmt, dtype=torch.int32, device=DEV), guard[:rows])
    assert out.data_ptr() == guard.data_ptr()
    got = guard.cpu().numpy()
    assert np.isnan(got[rows]).all(), "the ingress wrote past the batch"
    return got[:rows]


@pytest.mark.parametrize("rotation", [0, 1, 2])
@pytest.mark.parametrize("F", SIZES)
def test_ingress_equals_the_numpy_formula_bit_for_bit(F, rotation):
    fmt = _rot(FORMATS, rotation)
    rng = np.random.default_rng(1000 * F + rotation)
    # random BYTES everywhere: reserved header bytes and padding hold garbage, f32 payloads hold every kind of bit pattern (NaNs too)
    staged = rng.integers(0, 256, (B, SL.record_stride(F)), dtype=np.uint8)
    for present in ([1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [7, -1, 1 << 30]):           # present is "non-zero"
        staged[:, :4].view("<i4")[:, 0] = present
        want = SL.ingress_reference(staged, fmt, F)
        got = _ingress(staged, fmt, F)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (F, fmt, present)
        for b in range(B):
            if present[b] == 0 or fmt[b] < 0:
                assert not got[b].view(np.int32).any(), "a row without a frame, or a free row, is exact zeros"


def test_ingress_every_s16_value_once():
    F = 65536
    rng = np.random.default_rng(3)
    staged = rng.integers(0, 256, (2, SL.record_stride(F)), dtype=np.uint8)
    staged[:, :4].view("<i4")[:, 0] = 1
    values = rng.permutation(np.arange(-32768, 32768)).astype("<i2")
    staged[0, 16:16 + 2 * F] = np.frombuffer(values.tobytes(), dtype=np.uint8)
    fmt = [SL.FMT_S16, SL.FMT_F32]
    got = _ingress(staged, fmt, F, rows=2)
    assert np.array_equal(got[0, 0], values.astype(np.float32) / 32768.0)
    assert sorted(got[0, 0].tolist()) == [v / 32768.0 for v in range(-32768, 32768)]
    assert np.array_equal(got.view(np.int32), SL.ingress_reference(staged, fmt, F).view(np.int32))


def test_refusals():
    F = 5
    REC = SL.record_stride(F)
    fmt = torch.zeros(B, dtype=torch.int32, device=DEV)
    rec = torch.zeros(B, REC, dtype=torch.uint8, device=DEV)
    pcm = torch.zeros(B, 1, F, device=DEV)
    tokens = torch.zeros(B, 9, dtype=torch.long, device=DEV)
    off = torch.zeros(B, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_ingress(rec.cpu(), fmt, pcm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_egress(pcm.cpu(), tokens, off, 1, fmt, rec)
    with pytest.raises(ValueError, match="REC"):
        ops.frame_ingress(rec[:, :REC - 16].contiguous(), fmt, pcm)          # a record too short for the frame
    with pytest.raises(ValueError, match="offset_dev"):
        ops.frame_egress(pcm, tokens, off[:1], 1, fmt, rec)                  # a scalar session's single counter
    with pytest.raises(TypeError):
        ops.frame_egress(pcm, tokens.int(), off, 1, fmt, rec)
