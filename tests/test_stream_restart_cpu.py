"""Host side of per-stream sessions (no GPU): what is refused, that the scalar kernel wrappers still refuse position vectors, the
pipeline's restart schedule as a pure function, and the condition the GPU identity test rests on -- the oracle's own greedy decision
margins on the LM inputs of tests/helpers/stream_restart.py are at least 1e-4."""
import inspect

import pytest
import torch

from rstnet_amd import ops, synth
from rstnet_amd.codec import transformer as CT
from rstnet_amd.codec.audio_resample import StreamResampler
from rstnet_amd.codec.streaming import check_rows
from rstnet_amd.lm.model import LMGen, LMModel
from rstnet_amd.pipeline import restart_schedule
from tests.helpers import stream_restart as R


# ---- refusals

def _tiny_gen():
    cfg = dict(R.CFG)
    return LMGen(LMModel.from_state_dict(R.lm_state(), cfg), use_sampling=False), cfg


def test_prefill_on_a_per_stream_session_is_refused():
    gen, cfg = _tiny_gen()
    Ki = cfg["n_q"] - cfg["dep_q"]
    user, own = torch.zeros(2, Ki, 3, dtype=torch.long), torch.zeros(2, cfg["dep_q"] + 1, 3, dtype=torch.long)
    with gen.streaming(2, per_stream=True):
        state = gen._streaming_state
        assert tuple(state.offset_dev.shape) == (2,) and state.frames == [0, 0]
        tst = gen.lm_model.transformer._streaming_state
        assert tst.per_stream and tuple(tst.pos.shape) == (2,)
        assert state.depth.pos.numel() == 1 and not state.depth.per_stream, "the depth rings restart every frame for all streams: scalar"
        with pytest.raises(ValueError, match="per-stream"):
            gen.prefill(user, own)
    # the flag belongs to the session, not to the model: the next plain session is a scalar one
    with gen.streaming(2):
        assert gen._streaming_state.frames is None and gen._streaming_state.offset_dev.numel() == 1
        assert not gen.lm_model.transformer._streaming_state.per_stream
        with pytest.raises(ValueError, match="per-stream session"):
            gen.reset_streams([0])


def test_rows_out_of_range_are_refused():
    assert check_rows([2, 0, 2], 3) == [0, 2]
    for bad in ([3], [-1], [0, 7]):
        with pytest.raises(ValueError, match="outside the batch"):
            check_rows(bad, 3)
    gen, _ = _tiny_gen()
    with gen.streaming(3, per_stream=True):
        with pytest.raises(ValueError, match="outside the batch"):
            gen.reset_streams([3])
        gen.reset_streams([])           # nothing to do is not an error
    rs = StreamResampler(48000, 24000, 1920, 3, "cpu")
    assert tuple(rs.fresh.shape) == (3, 1) and bool(rs.fresh.all())
    with pytest.raises(ValueError, match="outside the batch"):
        rs.reset_rows([3])
    rs.fresh.fill_(False)
    rs.buf.fill_(1.0)
    rs.reset_rows([1])
    assert rs.fresh[:, 0].tolist() == [False, True, False]
    assert float(rs.buf[1].abs().max()) == 0.0 and bool((rs.buf[[0, 2]] == 1.0).all())


def test_codec_session_on_an_unserved_shape_is_refused():
    """Head size 16 is outside the one-launch attention step (32 / 64 / 128): a per-stream session cannot open, a scalar one can (it
    has the two-launch fallback)."""
    tr = CT.ProjectedTransformer(input_dimension=32, output_dimensions=(32,), d_model=32, num_heads=2, num_layers=1, causal=True,
                                 context=6, positional_embedding="rope", dim_feedforward=64, layer_scale=0.01, gating="none", norm="layer_norm")
    assert not ops.attention_step_serves(1, 16, 6) and ops.attention_step_serves(1, 64, 6)
    with pytest.raises(ValueError, match="per-stream session"):
        with tr.streaming(3, per_stream=True):
            pass
    assert tr.transformer._streaming_state is None and all(ly.self_attn._streaming_state is None for ly in tr.transformer.layers), \
        "a refused session leaves nothing half open"
    with tr.streaming(3):
        st = tr.transformer._streaming_state
        assert st.offset.numel() == 1
        with pytest.raises(ValueError, match="per-stream session"):
            st.reset_rows([0])
    ok = CT.ProjectedTransformer(input_dimension=128, output_dimensions=(128,), d_model=128, num_heads=2, num_layers=1, causal=True,
                                 context=6, positional_embedding="rope", dim_feedforward=64, layer_scale=0.01, gating="none", norm="layer_norm")
    with ok.streaming(3, per_stream=True):
        assert tuple(ok.transformer._streaming_state.offset.shape) == (3,)
        assert tuple(ok.transformer.layers[0].self_attn._streaming_state.offset.shape) == (3,)


# ---- scalar wrappers

SCALAR_WRAPPERS = ["attention_step", "attention", "rope_split", "gemv_attn", "lm_rope_append", "temporal_decode_frame", "codec_transformer_frame"]


@pytest.mark.parametrize("name", SCALAR_WRAPPERS)
def test_scalar_wrappers_still_refuse_a_vector(name):
    src = inspect.getsource(getattr(ops, name))
    assert f'_shared_pos(pos_dev, "{name}")' in src, f"ops.{name} no longer refuses a per-stream position vector"


def test_shared_pos_refuses_and_the_per_stream_wrapper_wants_a_vector():
    with pytest.raises(ValueError, match="one position for all streams"):
        ops._shared_pos(torch.zeros(3, dtype=torch.long), "attention_step")
    ops._shared_pos(torch.zeros(1, dtype=torch.long), "attention_step")
    assert "rst_attention_step_ps_f32" in inspect.getsource(ops.attention_step_ps)
    assert "_shared_pos" not in inspect.getsource(ops.attention_step_ps)


# ---- the host schedule of a restart, by hand

def test_restart_schedule_by_hand():
    # max_delay 1, three streams, all past their delay, nobody restarted: everyone valid, nothing to reset
    assert restart_schedule([5, 5, 5], [], 1) == ([], [0, 1, 2], [])
    # stream 1 restarted just now (frames 0, awaiting its second decoder-side reset): its frame 0 is inside the delay
    assert restart_schedule([5, 0, 5], [1], 1) == ([], [0, 2], [1])
    # next frame: stream 1 has stepped max_delay frames -> this frame gives its first valid output: reset its decoder side now, valid after
    assert restart_schedule([6, 1, 6], [1], 1) == ([1], [0, 1, 2], [])
    # and then it is an ordinary stream
    assert restart_schedule([7, 2, 7], [], 1) == ([], [0, 1, 2], [])
    # session start: nobody valid at frame 0, all valid from frame max_delay on; no second reset for streams that were never restarted
    assert restart_schedule([0, 0], [], 1) == ([], [], [])
    assert restart_schedule([1, 1], [], 1) == ([], [0, 1], [])
    # a longer delay counts down one frame at a time, per stream; two restarts at different frames keep their own clocks
    assert restart_schedule([9, 0, 2], [1, 2], 3) == ([], [0], [1, 2])
    assert restart_schedule([10, 1, 3], [1, 2], 3) == ([2], [0, 2], [1])
    assert restart_schedule([11, 2, 4], [1], 3) == ([], [0, 2], [1])
    assert restart_schedule([12, 3, 5], [1], 3) == ([1], [0, 1, 2], [])
    # a stream restarted again inside its delay starts its countdown again
    assert restart_schedule([4, 0], [1], 2) == ([], [0], [1])
    assert restart_schedule([5, 1], [1], 2) == ([], [0], [1])
    assert restart_schedule([6, 0], [1], 2) == ([], [0], [1])          # (reset once more before this frame)
    assert restart_schedule([7, 1], [1], 2) == ([], [0], [1])
    assert restart_schedule([8, 2], [1], 2) == ([1], [0, 1], [])


def test_validity_countdown_of_the_scenario():
    """The GPU scenario on the host: stream 2 is invalid for exactly max_delay frames after its reset."""
    max_delay = max(R.CFG["delays"])
    frames, awaiting, invalid = [0] * R.B, [], []
    for f in range(R.FRAMES):
        if f == R.RESET_FRAME:
            frames[R.RESET_ROW], awaiting = 0, [R.RESET_ROW]
        reset_now, valid, awaiting = restart_schedule(frames, awaiting, max_delay)
        assert reset_now == ([R.RESET_ROW] if f == R.RESET_FRAME + max_delay else [])
        invalid.append([b for b in range(R.B) if b not in valid])
        frames = [n + 1 for n in frames]
    assert invalid[:max_delay] == [[0, 1, 2]] * max_delay
    assert invalid[R.RESET_FRAME:R.RESET_FRAME + max_delay] == [[R.RESET_ROW]] * max_delay
    assert all(not x for f, x in enumerate(invalid) if f >= max_delay and not R.RESET_FRAME <= f < R.RESET_FRAME + max_delay)


# ---- the condition of the GPU identity test: the oracle's own margins

def test_oracle_margins_on_the_restart_scenario():
    runs, margin = R.oracle_runs()
    print(f"restart scenario: {len(runs)} conversations, smallest greedy decision margin {margin:.3e}")
    assert set(runs) == {(0, 0), (1, 0), (R.RESET_ROW, 0), (R.RESET_ROW, R.RESET_FRAME)}
    assert margin >= R.MARGIN
