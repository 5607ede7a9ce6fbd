"""Host side of the device sample-rate conversion: the fp64 reference and its bound (tests/helpers/resample_ref.py) against the
existing host ``resample``, the teeth of that bound, the stream geometry and the three-operation step restated on the host, the
server's rate arithmetic, and the grouping of ``offline.tokenize_list(..., resample="device")`` with a recording stand-in."""
import inspect
import os
import wave

import numpy as np
import pytest
import torch

from rstnet_amd import server as S
from rstnet_amd.codec import audio_resample as AR
from rstnet_amd.codec import offline
from tests.helpers import resample_ref as R

LENGTHS = [1, 5, 1000, 7777]


def _signal(T, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.1 * torch.randn(T, generator=g)


@pytest.mark.parametrize("orig,new", R.PAIRS)
def test_host_resample_is_within_the_bound_of_ref64(orig, new):
    o, n = R.reduced(orig, new)
    L = R.table(o, n)[0].shape[1]
    for T in LENGTHS:
        x = _signal(T, T + orig)
        y64, a64 = R.ref64(x, orig, new)
        got = AR.resample(x, orig, new)
        assert got.shape == (-(-n * T // o),)
        R.check(got, y64, a64, L, f"{orig}->{new} T={T}")


@pytest.mark.parametrize("orig,new", R.PAIRS)
def test_the_bound_has_teeth(orig, new):
    """Three wrong variants of the reference -- phase rows reversed, ``lead`` off by one, last tap dropped -- each break the bound
    against the right one on the same inputs (T = 1000 and 7777).  Two of them need a word.  "Last tap" is the last tap that carries
    weight: ``width`` is rounded up and the Hann window closes at the 6th zero crossing, so the last column of every table here is
    identically zero (asserted below) and the ones next to it are smaller than fp32 rounding of the sum -- dropping those computes
    the same values, and no bound on rounding error can or should tell.  The variant zeroes the last column whose largest weight is
    above ten times the bound's own relative size ``(L + 1) * 2^-24`` (the weights are of order one).  And with a single phase
    (``n == 1``: 48 -> 24 kHz, 24 -> 8 kHz) reversing the phase rows is the identity: that variant is checked where ``n > 1``."""
    o, n = R.reduced(orig, new)
    filt, width = R.table(o, n)
    L = filt.shape[1]
    for T in (1000, 7777):
        x = _signal(T, T + orig)
        T_out = -(-n * T // o)
        y64, a64 = R.contract64(x, filt, o, n, width, T_out)
        assert not filt[:, -1].any()
        last = int((filt.abs().amax(0) > 10 * (L + 1) * 2.0 ** -24).nonzero().max())
        dropped = filt.clone()
        dropped[:, last] = 0
        wrong = {"phases reversed": R.contract64(x, filt.flip(0), o, n, width, T_out)[0],
                 "lead + 1": R.contract64(x, filt, o, n, width + 1, T_out)[0],
                 "last tap dropped": R.contract64(x, dropped, o, n, width, T_out)[0]}
        if n == 1:
            assert torch.equal(wrong.pop("phases reversed"), y64)
        for name, y in wrong.items():
            assert R.violates(y.float(), y64, a64, L), f"{orig}->{new} T={T}: the variant `{name}` passes the bound"
        assert not R.violates(y64.float(), y64, a64, L)


def test_stream_geometry_values():
    frame_in = {8000: 640, 16000: 1280, 32000: 2560, 44100: 3528, 48000: 3840, 22050: 1764, 11025: 882}
    for rate, want in frame_in.items():
        for orig, new, f_out, f_in in ((rate, 24000, 1920, want), (24000, rate, want, 1920)):
            o, n, width, L, q, hist, got_in, delay = AR.stream_geometry(orig, new, f_out)
            assert (o, n) == R.reduced(orig, new) and got_in == f_in
            kernel, w = AR.sinc_kernel(o, n)
            assert width == w and L == kernel.shape[-1] == 2 * width + o
            assert q == -(-width // o) and hist == q * o + width and delay == q * n
            assert hist <= 334 and hist < got_in and delay <= 320, (orig, new, hist, delay)
    assert AR.stream_geometry(24000, 24000, 1920) == (1, 1, 0, 1, 0, 0, 1920, 0)
    assert AR.stream_geometry(7000, 24000, 1920)[6] == 560          # 7 : 24, and 24 divides 1920: servable
    for rate in (7001, 12345, 22051):                               # a 1920-sample frame is not a whole number of samples there
        with pytest.raises(ValueError):
            AR.stream_geometry(rate, 24000, 1920)
    with pytest.raises(ValueError):
        AR.stream_geometry(24000, 12345, 987)


@pytest.mark.parametrize("orig,new,frame_out", [(8000, 24000, 1920), (44100, 24000, 1920), (48000, 24000, 1920), (24000, 16000, 1280),
                                                (24000, 44100, 3528), (24000, 11025, 882), (24000, 24000, 1920)])
def test_three_operation_step_equals_the_streaming_definition(orig, new, frame_out):
    frames = 4
    hs = R.HostStream(orig, new, frame_out)
    x = _signal(frames * hs.frame_in, orig + new)
    got = torch.cat([hs.step(x[f * hs.frame_in:(f + 1) * hs.frame_in]) for f in range(frames)])
    if orig == new:
        assert torch.equal(got, x.double())
        return
    whole, a64 = R.ref64(x, orig, new)
    want = R.stream_ref(whole, hs.delay_out, frames * frame_out)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(a64.max())


def test_device_table_is_the_transposed_host_table():
    t = AR.device_table(147, 80, "cpu")
    kernel, _ = AR.sinc_kernel(147, 80)
    assert t.shape == (kernel.shape[-1], 80) and t.is_contiguous() and torch.equal(t, kernel[:, 0, :].t())
    assert AR.device_table(147, 80, "cpu") is t


def test_library_tile_and_argument_refusals_need_no_gpu():
    """The tile size Python exports is the library's, and the argument checks answer before any launch."""
    import ctypes
    from rstnet_amd import _lib, ops
    lib = _lib.lib()
    assert lib.rst_version() >= 126
    slab = ctypes.c_int(-1)
    assert lib.rst_resample_plan(147, 80, 306, ctypes.byref(slab)) == ops.RESAMPLE_TILE and slab.value > 0
    assert lib.rst_resample_plan(48, 1, 630, ctypes.byref(slab)) == ops.RESAMPLE_TILE and slab.value == 0      # span too long for LDS
    assert ops.resample_staged(320, 147, 348) and not ops.resample_staged(48, 1, 630)
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args, word in (((p, 0, 8, 8, None, p, 0, 1, 1, 0, p, 8, None, 1, 8, None), "o, n, L"),
                       ((p, 0, 8, 8, None, p, 1, 0, 1, 0, p, 8, None, 1, 8, None), "o, n, L"),
                       ((p, 0, 8, 8, None, p, 1, 1, 0, 0, p, 8, None, 1, 8, None), "o, n, L"),
                       ((p, 0, 8, 8, None, p, 1, 1, 1, -1, p, 8, None, 1, 8, None), "lead"),
                       ((p, 0, 8, 8, None, p, 1, 1, 1, 0, p, 8, None, 1, -1, None), "negative size"),
                       ((None, 0, 8, 8, None, p, 1, 1, 1, 0, p, 8, None, 1, 8, None), "null input"),
                       ((p, 0, 8, 8, None, p, 1, 1, 1, 0, None, 8, None, 1, 8, None), "null output"),
                       ((p, 0, 8, 8, None, None, 2, 1, 4, 0, p, 8, None, 1, 4, None), "null filter"),
                       ((p, 2, 8, 8, None, p, 1, 1, 1, 0, p, 8, None, 1, 8, None), "x_dtype")):
        assert lib.rst_resample_sinc(*args) < 0
        assert word in lib.rst_last_error().decode(), (word, lib.rst_last_error())


# ---- server: rate arithmetic and the 400 path ------------------------------------------------------------------------------------

def test_client_geometry():
    assert S.client_geometry(None, 24000, 1920) == (24000, 1920)
    assert S.client_geometry("24000", 24000, 1920) == (24000, 1920)
    for sr, frame in ((8000, 640), (16000, 1280), (44100, 3528), (48000, 3840), (11025, 882)):
        assert S.client_geometry(str(sr), 24000, 1920) == (sr, frame)
    assert S.client_geometry("7000", 24000, 1920) == (7000, 560) and S.client_geometry("384000", 24000, 1920) == (384000, 30720)
    # no whole-sample frame; not a rate; so low that the history outgrows a frame (25, 100, 150 Hz have whole-sample frames); above 16 x
    # the codec's rate; ratios whose tables are out of proportion (47975 Hz = 1919 : 960)
    for bad in ("7001", "12345", "0", "-48000", "fast", "44100.0", "25", "100", "150", "2400000000", "2399999975", "408000", "47975"):
        with pytest.raises(ValueError):
            S.client_geometry(bad, 24000, 1920)


class _Mimi:
    sample_rate, frame_rate = 24000, 12.5

    def streaming_forever(self, b):
        pass

    def reset_streaming(self):
        pass


class _Gen(_Mimi):
    pass


def test_bad_sr_is_answered_with_400_before_the_upgrade():
    import asyncio
    from aiohttp.test_utils import TestClient, TestServer

    async def scenario():
        st = S.ServerState(_Mimi(), None, "cpu", lm_gen=_Gen())
        client = TestClient(TestServer(S.make_app(st)))
        await client.start_server()
        try:
            out = []
            for q in ("sr=7001", "sr=fast", "sr=48000&pcm=nope", "sr=100", "sr=2400000000"):
                r = await client.get("/api/chat?" + q)
                out.append((r.status, await r.text()))
            return out
        finally:
            await client.close()

    loop = asyncio.new_event_loop()
    try:
        out = loop.run_until_complete(scenario())
    finally:
        loop.close()
    assert [s for s, _ in out] == [400] * 5
    assert "history" in out[3][1] and "2400000000" in out[4][1]
    assert "7001" in out[0][1] and "fast" in out[1][1] and "nope" in out[2][1]


# ---- offline: grouping by rate, int16 hand-over, order ----------------------------------------------------------------------------

class _Recorder:
    def __init__(self):
        self.calls = []

    def tokenize_batch(self, wavs, sample_rate, max_batch_seconds, **kw):
        self.calls.append(([(w.dtype, w.numel()) for w in wavs], sample_rate, max_batch_seconds, kw))
        return [torch.full((8, 1), w.numel() % 1000, dtype=torch.int16) for w in wavs]


def _write_wav(path, x, sr, width=2):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(width)
        w.setframerate(sr)
        scale, dt = (32767, "<i2") if width == 2 else (2147483647, "<i4")
        w.writeframes((np.clip(x, -1, 1) * scale).astype(dt).tobytes())


def _corpus(tmp_path):
    g = np.random.default_rng(0)
    spec = [("a", 16000, 2, 1601), ("b", 44100, 4, 2203), ("c", 16000, 2, 801), ("d", 24000, 2, 1203), ("e", 44100, 4, 1102), ("f", 16000, 2, 3004)]
    items = []
    for key, sr, width, T in spec:
        p = os.path.join(tmp_path, key + ".wav")
        _write_wav(p, 0.3 * g.standard_normal(T), sr, width)
        items.append((key, p))
    items.insert(2, ("missing", os.path.join(tmp_path, "nope.wav")))
    return spec, items


def test_tokenize_list_device_groups_by_rate_and_hands_over_int16(tmp_path):
    spec, items = _corpus(tmp_path)
    tok, skipped = _Recorder(), []
    out = offline.tokenize_list(tok, items, chunk_size=4, max_batch_seconds=7.0, skipped=skipped, resample="device")
    assert list(out) == [k for k, *_ in spec] and skipped == ["missing"]                       # input order, bad file skipped
    for key, sr, width, T in spec:
        assert int(out[key][0, 0]) == T % 1000                                                  # samples at the FILE's rate reached the tokenizer
    # chunk 1 = a, b, (missing), c ; chunk 2 = d, e, f: one call per rate within a chunk
    seen = [(sr, rows) for rows, sr, _, _ in tok.calls]
    assert seen == [(16000, [(torch.int16, 1601), (torch.int16, 801)]), (44100, [(torch.float32, 2203)]),
                    (24000, [(torch.int16, 1203)]), (44100, [(torch.float32, 1102)]), (16000, [(torch.int16, 3004)])]
    assert all(mbs == 7.0 and kw == {"resample": "device"} for _, _, mbs, kw in tok.calls)


def test_tokenize_list_host_calls_the_tokenizer_as_before(tmp_path):
    spec, items = _corpus(tmp_path)

    class Strict:       # today's signature: no further keyword is accepted
        def __init__(self):
            self.calls = []

        def tokenize_batch(self, wavs, sample_rate, max_batch_seconds):
            self.calls.append(([w.dtype for w in wavs], [w.numel() for w in wavs], sample_rate, max_batch_seconds))
            return [torch.zeros(8, 1, dtype=torch.int16) for _ in wavs]

    for kw in ({}, {"resample": "host"}):
        tok = Strict()
        out = offline.tokenize_list(tok, items, chunk_size=4, max_batch_seconds=7.0, **kw)
        assert list(out) == [k for k, *_ in spec]
        assert [c[2:] for c in tok.calls] == [(24000, 7.0), (24000, 7.0)]
        assert all(d == torch.float32 for c in tok.calls for d in c[0])
        assert tok.calls[0][1] == [-(-24000 * 1601 // 16000), -(-24000 * 2203 // 44100), -(-24000 * 801 // 16000)]
    with pytest.raises(ValueError):
        offline.tokenize_list(Strict(), items, resample="gpu")


def test_read_audio_raw(tmp_path):
    x = np.linspace(-0.9, 0.9, 501)
    p16, p32 = os.path.join(tmp_path, "a16.wav"), os.path.join(tmp_path, "a32.wav")
    _write_wav(p16, x, 16000, 2)
    _write_wav(p32, x, 16000, 4)
    raw, sr = offline.read_audio(p16, raw=True)
    assert sr == 16000 and raw.dtype == torch.int16 and torch.equal(raw.float() / 32768.0, offline.read_audio(p16)[0])
    assert offline.read_audio(p32, raw=True)[0].dtype == torch.float32
    assert "raw" in inspect.signature(offline.read_audio).parameters


def test_tokenizer_and_pipeline_signatures_default_to_the_host_route():
    from rstnet_amd.codec.tokenizer import MimiTokenizer
    from rstnet_amd.pipeline import StreamingPipeline
    assert inspect.signature(MimiTokenizer.tokenize_batch).parameters["resample"].default == "host"
    assert inspect.signature(offline.tokenize_list).parameters["resample"].default == "host"
    assert inspect.signature(StreamingPipeline.__init__).parameters["client_rate"].default is None


def test_stream_pair_geometry_refuses_before_anything_is_built(monkeypatch):
    """Every rate ``client_geometry`` lets through constructs both resamplers' geometry with ``hist < frame_in`` and a bounded table;
    what it refuses, it refuses without building a filter table."""
    def no_table(*a, **k):
        raise AssertionError("a filter table was built during validation")
    monkeypatch.setattr(AR, "sinc_kernel", no_table)
    served = 0
    for rate in list(range(25, 4000, 25)) + list(range(4000, 400000, 1975)) + [8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000]:
        try:
            frame = AR.stream_pair_geometry(rate, 24000, 1920)
        except ValueError:
            continue
        served += 1
        for orig, new, f_out in ((rate, 24000, 1920), (24000, rate, frame)):
            o, n, width, L, q, hist, frame_in, delay = AR.stream_geometry(orig, new, f_out)
            assert hist < frame_in and L * n <= AR.STREAM_MAX_TABLE and frame_in <= AR.STREAM_MAX_FRAME_RATIO * 1920
    assert served >= 8
    for rate in (8000, 11025, 16000, 22050, 32000, 44100, 48000):
        AR.stream_pair_geometry(rate, 24000, 1920)


def test_device_table_cache_is_bounded():
    AR._device_tables.clear()
    for o in range(2, 2 + AR.DEVICE_TABLES_MAX + 5):
        AR.device_table(o, 1, "cpu")
    assert len(AR._device_tables) == AR.DEVICE_TABLES_MAX
    first = AR.device_table(10, 1, "cpu")
    assert AR.device_table(10, 1, "cpu") is first


def test_pipeline_refuses_an_unservable_client_rate_in_its_constructor():
    """Before any streaming context is entered: nothing is left open by a refused rate."""
    from types import SimpleNamespace as NS
    from rstnet_amd.pipeline import StreamingPipeline
    entered = []
    mimi = NS(quantizer=NS(n_q=8), frame_hop=1920, streaming=lambda b: entered.append("mimi"))
    gen = NS(lm_model=NS(dep_q=8, num_codebooks=17, device="cpu"), streaming=lambda b: entered.append("lm"))
    for rate in (100, 7001, 2400000000):
        with pytest.raises(ValueError):
            StreamingPipeline(mimi, gen, 1, client_rate=rate)
    assert StreamingPipeline(mimi, gen, 1, client_rate=48000).client_frame == 3840
    assert StreamingPipeline(mimi, gen, 1).client_frame == 1920 and not entered
