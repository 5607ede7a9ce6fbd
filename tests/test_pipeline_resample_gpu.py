"""A live session at the client's sample rate: ``StreamingPipeline(client_rate=48000)`` must equal, bit for bit, the composition done
by hand -- ``StreamResampler`` in, a ``client_rate=None`` pipeline, ``StreamResampler`` out -- and ``ServerState.frame(chunk, sr)``
must equal that pipeline, as tests/test_server_gpu.py shows for the 24 kHz session.  Tiny LM and Mimi as that test builds them,
greedy sampling."""
import numpy as np
import pytest
import torch

from rstnet_amd import server as S
from rstnet_amd import synth
from rstnet_amd.codec.audio_resample import StreamResampler
from rstnet_amd.codec.loaders import get_mimi
from rstnet_amd.lm.model import LMGen, LMModel
from rstnet_amd.pipeline import StreamingPipeline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAME, RATE, CLIENT_FRAME = 1920, 48000, 3840


@pytest.fixture(scope="module")
def world():
    cfg = dict(synth.LM_TINY_16Q)
    mimi_sd = synth.mimi_state_dict(0)
    lm_sd = {k: v.to(DEV) for k, v in synth.lm_state_dict(cfg, seed=9).items()}

    def models():
        return get_mimi(mimi_sd, device=DEV), LMModel.from_state_dict(lm_sd, cfg)

    mimi, lm = models()
    frames = LMGen(lm, use_sampling=False).max_delay + 6
    g = torch.Generator().manual_seed(48)
    pcm48 = (0.1 * torch.randn(1, 1, frames * CLIENT_FRAME, generator=g)).to(DEV)

    # the number to meet: the pipeline at the client's rate
    want = []
    with StreamingPipeline(mimi, LMGen(lm, use_sampling=False), 1, client_rate=RATE) as pipe:
        assert pipe.client_frame == CLIENT_FRAME
        for f in range(frames):
            o = pipe.step(pcm48[:, :, f * CLIENT_FRAME:(f + 1) * CLIENT_FRAME].contiguous())
            want.append(None if o is None else o.cpu())
    return models, frames, pcm48, want


def _chunks(pcm, frames, size):
    return [pcm[:, :, f * size:(f + 1) * size].contiguous() for f in range(frames)]


def test_pipeline_at_client_rate_equals_the_hand_composition(world):
    models, frames, pcm48, want = world
    mimi, lm = models()
    rs_in = StreamResampler(RATE, 24000, FRAME, 1, DEV)
    rs_out = StreamResampler(24000, RATE, CLIENT_FRAME, 1, DEV)
    produced = 0
    with StreamingPipeline(mimi, LMGen(lm, use_sampling=False), 1) as pipe:
        for f, chunk in enumerate(_chunks(pcm48, frames, CLIENT_FRAME)):
            o = pipe.step(rs_in.step(chunk).clone())
            assert (o is None) == (want[f] is None), f
            if o is not None:
                got = rs_out.step(o)
                assert tuple(got.shape) == (1, 1, CLIENT_FRAME)
                assert torch.equal(got.cpu(), want[f]), f"frame {f}"
                produced += 1
    assert produced >= 6 and float(torch.cat([w for w in want if w is not None], -1).abs().max()) > 0


def test_server_frame_at_client_rate_equals_the_pipeline(world):
    models, frames, pcm48, want = world
    mimi, lm = models()
    st = S.ServerState(mimi, lm, DEV, use_sampling=False)
    st.warmup()                                      # four silent 24 kHz frames; the session below starts from reset states
    st.reset_session(RATE)
    got = []
    with torch.no_grad():
        for chunk in _chunks(pcm48, frames, CLIENT_FRAME):
            got += [p for p, _ in st.frame(chunk, RATE)]
    ref = [w[0, 0].numpy() for w in want if w is not None]
    assert len(got) == len(ref) >= 6
    for f, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == (CLIENT_FRAME,) and float(np.abs(a - b).max()) <= 1e-5 * max(1.0, float(np.abs(b).max())), f"frame {f}"
    # a second session at that rate starts from reset resamplers too
    st.reset_session(RATE)
    with torch.no_grad():
        again = []
        for chunk in _chunks(pcm48, frames, CLIENT_FRAME):
            again += [p for p, _ in st.frame(chunk, RATE)]
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_default_rate_pipeline_is_deterministic(world):
    """Sanity only (the existing tests pin this path): two ``client_rate=None`` sessions give the same samples."""
    models, frames, pcm48, _ = world
    pcm24 = pcm48[:, :, :frames * FRAME]
    runs = []
    for _ in range(2):
        mimi, lm = models()
        outs = []
        with StreamingPipeline(mimi, LMGen(lm, use_sampling=False), 1) as pipe:
            for chunk in _chunks(pcm24, frames, FRAME):
                o = pipe.step(chunk)
                if o is not None:
                    outs.append(o.cpu())
        runs.append(torch.cat(outs, -1))
    assert torch.equal(runs[0], runs[1])
