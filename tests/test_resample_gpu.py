"""rst_resample_sinc on the GPU: every output against the fp64 contract under the derived bound (tests/helpers/resample_ref.py) for
the twelve rate pairs, ragged rows aimed at the tile edges, fp32 and int16 inputs, strided rows, a NaN-filled output (the kernel
writes the zero tail itself); refusals; the streamed conversion against the whole-signal one bit for bit (eager, after a reset,
and replayed from a captured graph); and the tokenizer's device route against the single-utterance route on the same bits."""
import pytest
import torch

from rstnet_amd import _lib, ops, synth
from rstnet_amd.codec import audio_resample as AR
from tests.helpers import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = ops.RESAMPLE_TILE


def _lengths(o, n):
    """Input lengths of the issue: 1, o - 1, o, o + 1 and, for every output count TILE * k - 1, TILE * k, TILE * k + 1 (k = 1, 3),
    the shortest input that has that many outputs -> list of (in_len, out_len).  Where the rates skip a count (up-sampling:
    ``ceil(n * len / o)`` moves in steps) the row is cut to it through ``out_lengths``, which the contract allows."""
    rows = [(t, -(-n * t // o)) for t in (1, o - 1, o, o + 1)]
    for k in (1, 3):
        for cnt in (TILE * k - 1, TILE * k, TILE * k + 1):
            rows.append((-(-cnt * o // n), cnt))
    for t, cnt in rows:
        assert cnt <= -(-n * t // o)
    return rows


def _signal(T, seed, dtype, full_scale=False):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int16:
        if full_scale:
            return torch.tensor([32767, -32768], dtype=torch.int16)[torch.randint(0, 2, (T,), generator=g)]
        return (0.1 * torch.randn(T, generator=g) * 32768).round().clamp(-32768, 32767).to(torch.int16)
    return 0.1 * torch.randn(T, generator=g)


def _run_launch(o, n, lead, filt, filt_t, rows, dtype, seed, full_scale=False):
    """One launch over the ragged ``rows`` [(in_len, out_len)]: strided input rows, strided NaN-filled output rows, checked per
    element against the contract; -> worst error / bound."""
    B = len(rows)
    T_in = max(max(t for t, _ in rows), 1)
    T_out = max(c for _, c in rows) + 3                  # every row, the longest included, has a tail the kernel must zero
    xs = [_signal(t, seed + 17 * b, dtype, full_scale) for b, (t, _) in enumerate(rows)]
    big = torch.full((B, T_in + 5), 7 if dtype == torch.int16 else float("nan"), dtype=dtype)      # what lies behind a row must not be read
    for b, x in enumerate(xs):
        big[b, :x.numel()] = x
        if dtype == torch.float32:
            big[b, x.numel():T_in] = 3.0                 # inside the row but behind its length: must count as zero
    x_dev = big.to(DEV)[:, :T_in]
    y_big = torch.full((B, T_out + 7), float("nan"), device=DEV)
    in_len = torch.tensor([t for t, _ in rows], dtype=torch.int32, device=DEV)
    out_len = torch.tensor([c for _, c in rows], dtype=torch.int32, device=DEV)
    y = ops.resample_sinc(x_dev, in_len, filt_t, o, n, lead, T_out, out_lengths=out_len, out=y_big[:, :T_out])
    assert y.data_ptr() == y_big.data_ptr()
    got = y_big.cpu()
    assert torch.isnan(got[:, T_out:]).all(), "wrote behind a row of the output"
    worst = 0.0
    L = filt.shape[1]
    for b, (t, cnt) in enumerate(rows):
        y64, a64 = R.contract64(xs[b], filt, o, n, lead, cnt)
        worst = max(worst, R.check(got[b, :cnt], y64, a64, L, f"o={o} n={n} row {b} len {t}"))
        assert (got[b, cnt:T_out] == 0).all(), f"o={o} n={n} row {b}: the tail behind {cnt} outputs is not zero"
    return worst


def _sweep(orig, new, dtype, full_scale=False):
    o, n = R.reduced(orig, new)
    filt, width = R.table(o, n)
    filt_t = AR.device_table(o, n, DEV)
    rows = _lengths(o, n)
    longest = max(rows)
    others = [r for r in rows if r != longest and r != rows[0]]
    worst = 0.0
    for s, other in enumerate(others):                  # B = 3: a row of length 1, one of the other lengths, the longest row
        worst = max(worst, _run_launch(o, n, width, filt, filt_t, [rows[0], other, longest], dtype, 1000 * s + orig % 97, full_scale))
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16], ids=["f32", "s16"])
@pytest.mark.parametrize("orig,new", R.PAIRS)
def test_kernel_against_fp64_contract(orig, new, dtype):
    o, n = R.reduced(orig, new)
    assert ops.resample_staged(o, n, 2 * AR.filter_width(o, n) + o)           # the audio rates all stage their inputs in LDS
    worst = _sweep(orig, new, dtype)
    print(f"{orig}->{new} {dtype}: worst error / bound = {worst:.3f}")


def test_kernel_full_scale_s16():
    for orig, new in ((44100, 24000), (24000, 11025), (16000, 24000)):
        _sweep(orig, new, torch.int16, full_scale=True)


def test_kernel_without_lds_staging():
    """A ratio whose tile spans more input than the LDS slab holds takes the kernel's other route (inputs read from global memory):
    same contract, same bound."""
    orig, new = 48000, 1000
    o, n = R.reduced(orig, new)
    assert not ops.resample_staged(o, n, 2 * AR.filter_width(o, n) + o)
    filt, width = R.table(o, n)
    filt_t = AR.device_table(o, n, DEV)
    for dtype in (torch.float32, torch.int16):
        _run_launch(o, n, width, filt, filt_t, [(1, 1), (o * (TILE + 1), TILE + 1), (o * 2 * TILE - 5, 2 * TILE)], dtype, 5)


def test_equal_rates_convert_only():
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-32768, 32768, (3, 700), generator=g).to(torch.int16)
    lens = torch.tensor([700, 1, 257], dtype=torch.int32)
    y, out_len = AR.resample_device(x.to(DEV), lens.to(DEV), 24000, 24000)
    assert tuple(y.shape) == (3, 1, 700) and torch.equal(out_len.cpu(), lens)
    for b in range(3):
        want = torch.zeros(700)
        want[:lens[b]] = x[b, :lens[b]].float() / 32768.0
        assert torch.equal(y[b, 0].cpu(), want)


def test_resample_device_matches_host_resample_rows():
    """The whole-signal form: lengths, shapes, the zero tail, and each row against the host function through the shared bound."""
    orig, new = 44100, 24000
    o, n = R.reduced(orig, new)
    lens = [4410, 1, 3000]
    xs = [_signal(t, 40 + t, torch.float32) for t in lens]
    batch = torch.zeros(3, max(lens))
    for b, x in enumerate(xs):
        batch[b, :x.numel()] = x
    y, out_len = AR.resample_device(batch.to(DEV), torch.tensor(lens, dtype=torch.int32), orig, new)
    assert tuple(y.shape) == (3, 1, -(-n * max(lens) // o))
    assert out_len.dtype == torch.int32 and out_len.tolist() == [-(-n * t // o) for t in lens]
    L = R.table(o, n)[0].shape[1]
    for b, x in enumerate(xs):
        y64, a64 = R.ref64(x, orig, new)
        R.check(y[b, 0, :out_len[b]], y64, a64, L, f"row {b}")
        R.check(AR.resample(x, orig, new), y64, a64, L, f"host row {b}")
        assert (y[b, 0, out_len[b]:] == 0).all()


def test_refusals_are_runtime_errors_with_the_library_text():
    x = torch.zeros(2, 64, device=DEV)
    filt = torch.zeros(4, 1, device=DEV)
    with pytest.raises(RuntimeError, match="lead >= 0"):
        ops.resample_sinc(x, None, filt, 2, 1, -1, 32)
    with pytest.raises(RuntimeError, match="o, n, L >= 1"):
        ops.resample_sinc(x, None, filt, 0, 1, 0, 32)
    with pytest.raises(RuntimeError, match="negative size"):
        ops.resample_sinc(x, None, filt, 2, 1, 0, -1)
    with pytest.raises(RuntimeError, match="null filter"):
        ops.resample_sinc(x, None, None, 2, 1, 0, 32)
    with pytest.raises(_lib.RstError):
        ops.resample_sinc(x, None, torch.zeros(0, 1, device=DEV), 2, 1, 0, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_sinc(x.cpu(), None, filt.cpu(), 2, 1, 0, 32)


STREAM_RATES = [8000, 16000, 44100, 48000]


@pytest.mark.parametrize("direction", ["in", "out"])
@pytest.mark.parametrize("rate", STREAM_RATES)
def test_stream_equals_whole_signal_bit_for_bit(rate, direction):
    frames, B = 6, 2
    client_frame = AR.stream_geometry(rate, 24000, 1920)[6]
    orig, new, frame_out = (rate, 24000, 1920) if direction == "in" else (24000, rate, client_frame)
    rs = AR.StreamResampler(orig, new, frame_out, B, DEV)
    assert rs.hist < rs.frame_in and tuple(rs.buf.shape) == (B, rs.hist + rs.frame_in)
    g = torch.Generator().manual_seed(rate)
    x = (0.1 * torch.randn(B, frames * rs.frame_in, generator=g)).to(DEV)
    whole, _ = AR.resample_device(x, None, orig, new)
    want = R.stream_ref(whole[:, 0], rs.delay_out, frames * frame_out)
    assert want.abs().max() > 0.01

    def chunk(f):
        return x[:, None, f * rs.frame_in:(f + 1) * rs.frame_in].contiguous()

    def run():
        return torch.cat([rs.step(chunk(f))[:, 0].clone() for f in range(frames)], -1)

    state = (rs.buf.data_ptr(), rs.out.data_ptr())
    assert torch.equal(run(), want)
    rs.reset()
    assert torch.equal(run(), want), "after reset()"
    assert (rs.buf.data_ptr(), rs.out.data_ptr()) == state             # nothing is re-allocated

    # the step captured in a graph and replayed six times
    rs.reset()
    static_in = torch.zeros(B, 1, rs.frame_in, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = rs.step(static_in)
    rs.reset()                                                           # (a capture does not execute; start the session anyway)
    outs = []
    for f in range(frames):
        static_in.copy_(chunk(f))
        graph.replay()
        outs.append(static_out[:, 0].clone())
    assert torch.equal(torch.cat(outs, -1), want), "graph replay"


def test_stream_masks_the_pre_signal_outputs_whatever_they_hold():
    """The first ``delay_out`` outputs after a reset are +0 even when the first chunk starts with NaN / Inf (the whole-signal form has
    zeros there by definition), and only in that step."""
    rs = AR.StreamResampler(24000, 8000, 640, 2, DEV)
    chunk = torch.full((2, 1, rs.frame_in), 0.25, device=DEV)
    chunk[0, 0, 0], chunk[1, 0, 1] = float("nan"), float("-inf")
    head = rs.step(chunk)[:, 0, :rs.delay_out].clone()
    assert rs.delay_out > 0 and (head == 0).all() and not torch.signbit(head).any()
    again = rs.step(torch.full((2, 1, rs.frame_in), 0.25, device=DEV))[:, 0, :rs.delay_out]
    assert (again != 0).all()
    rs.reset()
    assert (rs.step(chunk)[:, 0, :rs.delay_out] == 0).all()


def test_tokenizer_device_route():
    from rstnet_amd.codec.mimi import MimiCodec
    from rstnet_amd.codec.tokenizer import MimiTokenizer
    tok = MimiTokenizer(MimiCodec.from_state_dict(synth.mimi_state_dict(0)).to(DEV))
    lens = [int(0.3 * 16000), int(0.5 * 16000), int(1.1 * 16000)]
    wavs = [_signal(t, 70 + i, torch.int16) for i, t in enumerate(lens)]
    got = tok.tokenize_batch([wavs[2], wavs[0], wavs[1]], 16000, resample="device")
    for w, codes in zip([wavs[2], wavs[0], wavs[1]], got):
        y, out_len = AR.resample_device(w[None].to(DEV), None, 16000, 24000)
        n24 = -(-3 * w.numel() // 2)
        assert int(out_len[0]) == n24
        single = tok.tokenize(y[..., :n24], 24000)
        assert codes.dtype == torch.int16 and tuple(codes.shape) == (8, -(-n24 // 1920))
        assert torch.equal(codes, single)
    # a small batch budget splits the batch and changes nothing
    split = tok.tokenize_batch([wavs[2], wavs[0], wavs[1]], 16000, max_batch_seconds=1.0, resample="device")
    assert all(torch.equal(a, b) for a, b in zip(got, split))
    # at 24 kHz the device route only moves the s16 -> f32 conversion: codes equal the host route's exactly
    host = tok.tokenize_batch([w.float() / 32768.0 for w in wavs], 24000)
    dev = tok.tokenize_batch(wavs, 24000, resample="device")
    dev_f32 = tok.tokenize_batch([w.float() / 32768.0 for w in wavs], 24000, resample="device")
    for a, b, c in zip(host, dev, dev_f32):
        assert torch.equal(a, b) and torch.equal(a, c)
