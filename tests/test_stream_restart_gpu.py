"""Per-stream sessions on the GPU: one position / frame counter / history seed per stream in every stateful module of the live frame,
so that single rows of a running batch can start over (``reset_streams``) while the others do not notice.

1. ``ops.attention_step_ps`` == ``ops.attention_step`` launched once per distinct position on copies of the same rings, bit for bit.
2. The token-ring kernels at per-stream frame counters == the scalar launches, one per counter.
3. ``ops.hist_seed``: flagged rows get the seed of a new ``StreamingConv1d`` session, the others keep their bytes.
4. ``MimiCodec`` (and a ``ProjectedTransformer`` alone, across its ring's wrap): a reset row == a new session, the others undisturbed.
5. ``LMGen``: the scenario of tests/helpers/stream_restart.py against the scalar session and the CPU oracle, with and without graphs.
6. ``StreamingPipeline(per_stream=True)``: == the scalar pipeline without a restart; with one, the restarted row == a new pipeline's
   and the composed oracles' (1e-3 relative, the bound of tests/test_e2e_gpu.py), under one frame graph that is never re-captured.

Equality with SCALAR sessions is asserted at three streams: at two the scalar codec takes the persistent transformer launch."""
import functools

import pytest
import torch

from oracle import lm_oracle as L
from oracle import mimi_oracle as O
from rstnet_amd import ops, synth
from rstnet_amd.codec import transformer as CT
from rstnet_amd.codec.conv import StreamingConv1d
from rstnet_amd.codec.mimi import MimiCodec
from rstnet_amd.codec.streaming import reset_stream_rows
from rstnet_amd.lm.model import LMGen, LMModel
from rstnet_amd.pipeline import StreamingPipeline
from tests.helpers import stream_restart as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRAME = 1920


def _bits(t: torch.Tensor) -> torch.Tensor:
    """fp32 as its bit patterns: equality that also holds NaN to NaN."""
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ 1: attention_step_ps

def _packed_index(row: torch.Tensor, k: torch.Tensor, Kp: int) -> torch.Tensor:
    """Element (row, k) of the few-row GEMM's packed fp32 operand (f32_packed_index of csrc/rst_common.h)."""
    return ((((row >> 5) * (Kp >> 3) + (k >> 3)) * 64) + (k & 1) * 32 + (row & 31)) * 4 + ((k & 7) >> 1)


@pytest.mark.parametrize("cap", [12, 250])
@pytest.mark.parametrize("T", [1, 2])
def test_attention_step_ps_equals_scalar_launches(T, cap):
    D, H = 64, 2
    positions = [0, 1, cap - 1, cap, 3 * cap + 5]
    B = len(positions)
    g = torch.Generator().manual_seed(100 * cap + T)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(DEV)
    k0, v0 = torch.randn(B, H, cap, D, generator=g), torch.randn(B, H, cap, D, generator=g)
    # what no stream may read: slots at or past the used part of a ring.  Stream 0 (position 0) uses T slots, stream 1 uses 1 + T
    for b in (0, 1):
        k0[b, :, cap - 1] = float("nan")
        v0[b, :, cap - 2:] = float("nan")
    k0, v0 = k0.to(DEV), v0.to(DEV)
    pos = torch.tensor(positions, device=DEV, dtype=torch.long)
    kp, vp = k0.clone(), v0.clone()
    out = ops.attention_step_ps(qkv, H, kp, vp, pos, context=cap, rope=True)
    assert bool(torch.isfinite(out).all()), "a stream read a slot it must not see"
    for b, p in enumerate(positions):
        ks, vs = k0.clone(), v0.clone()
        ref = ops.attention_step(qkv, H, ks, vs, torch.tensor([p], device=DEV, dtype=torch.long), context=cap, rope=True)
        assert torch.equal(out[b], ref[b]), (b, p)
        assert torch.equal(_bits(kp[b]), _bits(ks[b])) and torch.equal(_bits(vp[b]), _bits(vs[b])), (b, p)
    assert pos.tolist() == positions, "the step reads the positions; its caller moves them"


def test_attention_step_ps_packed_output():
    D, H, T, cap = 64, 2, 2, 12
    positions = [0, 1, cap - 1, cap, 3 * cap + 5]
    B, E = len(positions), H * D
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, T, 3 * E, generator=g).to(DEV)
    k0, v0 = torch.randn(B, H, cap, D, generator=g).to(DEV), torch.randn(B, H, cap, D, generator=g).to(DEV)
    pos = torch.tensor(positions, device=DEV, dtype=torch.long)
    ka, va, kb, vb = k0.clone(), v0.clone(), k0.clone(), v0.clone()
    plain = ops.attention_step_ps(qkv, H, ka, va, pos, context=cap, rope=True)
    packed = ops.attention_step_ps(qkv, H, kb, vb, pos, context=cap, rope=True, out_packed=True)
    assert isinstance(packed, ops.PackedRows) and packed.shape == (B, T, E) and tuple(packed.xp.shape) == (32, E)
    rows, cols = torch.meshgrid(torch.arange(32, device=DEV), torch.arange(E, device=DEV), indexing="ij")
    want = torch.zeros(32, E, device=DEV)
    want[:B * T] = plain.view(B * T, E)                      # (the rows past B * T read as zeros in the consumer)
    got = packed.xp.reshape(-1)[_packed_index(rows, cols, E)]
    assert torch.equal(got, want)
    assert torch.equal(ka, kb) and torch.equal(va, vb)


# ------------------------------------------------------------------------------------------------------------ 2: the token ring

def test_ring_kernels_at_per_stream_offsets():
    K, Ki, n_out = 5, 2, 3
    delays = [0, 0, 1, 0, 2]
    max_delay, CT = 2, 4
    offsets = [0, 1, max_delay, max_delay + 1, CT + 3]
    B = len(offsets)
    g = torch.Generator().manual_seed(11)
    cache0 = torch.randint(0, 30, (B, K, CT), generator=g).to(DEV)
    user = torch.randint(0, 30, (B, Ki), generator=g).to(DEV)
    tokens = torch.randint(0, 30, (B, n_out), generator=g).to(DEV)
    initial = torch.tensor([40, 41, 42, 43, 44], device=DEV)
    d32 = torch.tensor(delays, device=DEV, dtype=torch.int32)
    off = torch.tensor(offsets, device=DEV, dtype=torch.long)
    cache = cache0.clone()
    inp = ops.lm_ring_begin(cache, user, initial, d32, off, K - Ki)
    assert off.tolist() == offsets
    after_begin = cache.clone()
    out = ops.lm_ring_commit(cache, tokens, d32, off, max_delay)
    assert off.tolist() == [o + 1 for o in offsets], "every stream's counter moves by one, once"
    for b, o in enumerate(offsets):
        c, o1 = cache0.clone(), torch.tensor([o], device=DEV, dtype=torch.long)
        ref_in = ops.lm_ring_begin(c, user, initial, d32, o1, K - Ki)
        assert torch.equal(inp[b], ref_in[b]) and torch.equal(after_begin[b], c[b]), (b, o)
        ref_out = ops.lm_ring_commit(c, tokens, d32, o1, max_delay)
        assert int(o1) == o + 1
        assert torch.equal(out[b], ref_out[b]) and torch.equal(cache[b], c[b]), (b, o)
    # streams inside their delay got their initial tokens (offset <= delay_k), each by its own counter
    assert inp[0].tolist() == [40, 41, 42, 43, 44]
    assert inp[1].tolist()[2] == 42 and inp[1].tolist()[4] == 44 and inp[2].tolist()[4] == 44
    assert not set(inp[3].tolist() + inp[4].tolist()) & {40, 41, 42, 43, 44}


# ------------------------------------------------------------------------------------------------------------ 3: the history seed

@pytest.mark.parametrize("pad_mode", ["replicate", "constant"])
def test_hist_seed_matches_a_new_session(pad_mode):
    """The seed of ``StreamingConv1d.forward_nlc``'s first chunk: ``padding_total`` copies of the chunk's first step, or zeros (the module
    level, against a real new session, is the next test)."""
    B, C, T, k, s = 5, 24, 4, 4, 2
    torch.manual_seed(5)
    x = torch.randn(B, T, C, device=DEV)
    P = k - s
    seed = x[:, :1].expand(B, P, C).contiguous() if pad_mode == "replicate" else torch.zeros(B, P, C, device=DEV)
    hist0 = torch.randn(B, P, C, device=DEV)
    hist0[3, 0, 0] = float("nan")
    hist = hist0.clone()
    fresh = torch.tensor([0, 1, 0, 1, 1], device=DEV, dtype=torch.int32)
    ops.hist_seed(x, hist, fresh, replicate=pad_mode == "replicate")
    for b in range(B):
        assert torch.equal(_bits(hist[b]), _bits(seed[b] if b in (1, 3, 4) else hist0[b])), b
    assert fresh.tolist() == [0] * B
    ops.hist_seed(x, hist, fresh, replicate=pad_mode == "replicate")          # no flag: nothing moves
    assert torch.equal(_bits(hist[0]), _bits(hist0[0])) and torch.equal(_bits(hist[2]), _bits(hist0[2]))


def test_per_stream_conv_reseeds_a_reset_row_in_its_next_chunk():
    """The module level of the same: a replicate-padded per-stream convolution, row 1 reset after two chunks == a new session's row."""
    B, C, T = 3, 32, 4
    torch.manual_seed(6)
    conv = StreamingConv1d(C, 16, kernel_size=4, stride=2, causal=True, bias=False, pad_mode="replicate").to(DEV)
    xs = [torch.randn(B, T, C, device=DEV) for _ in range(4)]
    with conv.streaming(B):
        plain = [conv.forward_nlc(x) for x in xs]
    with conv.streaming(B, per_stream=True):
        got = [conv.forward_nlc(x) for x in xs[:2]]
        reset_stream_rows(conv, [1])
        got += [conv.forward_nlc(x) for x in xs[2:]]
        assert conv._streaming_state.fresh.tolist() == [0, 0, 0]
    with conv.streaming(B, per_stream=True):
        new = [conv.forward_nlc(x) for x in xs[2:]]
    for f in range(4):
        assert torch.equal(got[f][[0, 2]], plain[f][[0, 2]]), f
    assert torch.equal(got[0][1], plain[0][1]) and torch.equal(got[1][1], plain[1][1])
    assert torch.equal(got[2][1], new[0][1]) and torch.equal(got[3][1], new[1][1])
    assert not torch.equal(got[2][1], plain[2][1])


# ------------------------------------------------------------------------------------------------------------ 4: the codec

@functools.lru_cache(maxsize=1)
def _mimi():
    sd = synth.mimi_state_dict(0)
    return sd, MimiCodec.from_state_dict(sd).to(DEV)


def _codec_run(model, audio, codes, frames, reset_at=None, rows=(), per_stream=True, side="both"):
    """Encode and decode ``frames`` (a list of frame indices) in one session -> (codes [B, K, n], waveform [B, 1, n * FRAME])."""
    cs, ws = [], []
    with model.streaming(audio.shape[0], per_stream=per_stream):
        for f in frames:
            if f == reset_at:
                model.reset_streams(list(rows), side=side)
            cs.append(model.encode(audio[:, :, f * FRAME:(f + 1) * FRAME].contiguous()))
            ws.append(model.decode(codes[:, :, f:f + 1].contiguous()))
    return torch.cat(cs, -1), torch.cat(ws, -1)


def test_mimi_reset_row_equals_a_new_session():
    sd, model = _mimi()
    B, n = 3, 8
    audio = synth.synth_audio(B, n * FRAME, seed=31).to(DEV)
    card = sd["quantizer.rvq_first.vq.layers.0._codebook.embedding_sum"].shape[0]
    codes = torch.randint(0, card, (B, 8, n), generator=torch.Generator().manual_seed(32)).to(DEV)
    c_scalar, w_scalar = _codec_run(model, audio, codes, range(n), per_stream=False)
    c_plain, w_plain = _codec_run(model, audio, codes, range(n))
    c_got, w_got = _codec_run(model, audio, codes, range(n), reset_at=4, rows=[1])
    c_new, w_new = _codec_run(model, audio, codes, range(4, n))
    # a per-stream session nobody resets is the scalar session (three streams: both take the layer loop)
    assert torch.equal(c_plain, c_scalar) and torch.equal(w_plain, w_scalar)
    # encode
    assert torch.equal(c_got[[0, 2]], c_plain[[0, 2]]) and torch.equal(c_got[1, :, :4], c_plain[1, :, :4])
    assert torch.equal(c_got[1, :, 4:], c_new[1])
    # decode
    assert torch.equal(w_got[[0, 2]], w_plain[[0, 2]]) and torch.equal(w_got[1, :, :4 * FRAME], w_plain[1, :, :4 * FRAME])
    assert torch.equal(w_got[1, :, 4 * FRAME:], w_new[1])
    assert not torch.equal(w_got[1, :, 4 * FRAME:], w_plain[1, :, 4 * FRAME:]), "the reset changed nothing: the test shows nothing"
    # one side at a time
    c_enc, w_enc = _codec_run(model, audio, codes, range(n), reset_at=4, rows=[1], side="encoder")
    assert torch.equal(c_enc, c_got) and torch.equal(w_enc, w_plain)
    with model.streaming(B):
        with pytest.raises(ValueError, match="per-stream session"):
            model.reset_streams([0])


def test_projected_transformer_restart_across_the_wrap():
    """Two layers, a 6-slot ring, 10 one-position frames, stream 1 restarted at frame 3: from frame 6 on the undisturbed streams have
    wrapped while the restarted one fills its ring (over what its earlier conversation left there), and wraps itself at frame 9."""
    torch.manual_seed(8)
    tr = CT.ProjectedTransformer(input_dimension=128, output_dimensions=(128,), d_model=128, num_heads=2, num_layers=2, causal=True,
                                 context=6, positional_embedding="rope", dim_feedforward=256, layer_scale=0.05, gating="none",
                                 norm="layer_norm").to(DEV)
    B, n, at = 3, 10, 3
    xs = [torch.randn(B, 1, 128, device=DEV) for _ in range(n)]

    def run(frames, reset_at=None):
        ys = []
        with tr.streaming(B, per_stream=True), torch.no_grad():
            for f in frames:
                if f == reset_at:
                    reset_stream_rows(tr, [1])
                ys.append(tr.forward_nlc(xs[f])[0])
            offs = tr.transformer._streaming_state.offset.tolist()
        return torch.cat(ys, 1), offs

    plain, offs = run(range(n))
    assert offs == [n, n, n]
    got, offs = run(range(n), reset_at=at)
    assert offs == [n, n - at, n]
    new, _ = run(range(at, n))
    assert torch.equal(got[[0, 2]], plain[[0, 2]]) and torch.equal(got[1, :at], plain[1, :at])
    assert torch.equal(got[1, at:], new[1])
    assert not torch.equal(got[1, at:], plain[1, at:])


# ------------------------------------------------------------------------------------------------------------ 5: LMGen

@functools.lru_cache(maxsize=1)
def _tiny_lm():
    cfg = dict(R.CFG)
    return LMModel.from_state_dict({k: v.to(DEV) for k, v in R.lm_state().items()}, cfg)


def _lm_run(gen, user, per_stream, reset=True):
    outs, valid = [], []
    with gen.streaming(R.B, per_stream=per_stream), torch.no_grad():
        for f in range(R.FRAMES):
            if reset and f == R.RESET_FRAME:
                gen.reset_streams([R.RESET_ROW])
            o = gen.step(user[f].to(DEV))
            outs.append(None if o is None else o.cpu())
            valid.append(gen.stream_valid())
    return outs, valid


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "no_graphs"])
def test_lmgen_restart_matches_scalar_session_and_oracle(graphs, monkeypatch):
    if not graphs:
        monkeypatch.setenv("NO_CUDA_GRAPH", "1")
    gen = LMGen(_tiny_lm(), use_sampling=False)
    user = R.user_tokens()
    runs, margin = R.oracle_runs()
    assert margin >= R.MARGIN
    max_delay = gen.max_delay
    scalar, _ = _lm_run(gen, user, per_stream=False, reset=False)
    got, valid = _lm_run(gen, user, per_stream=True)
    with gen.streaming(R.B, per_stream=True):
        assert gen._streaming_state.graphed_frame.disable == (not graphs)
    everyone = list(range(R.B))
    others = [b for b in everyone if b != R.RESET_ROW]
    for f in range(R.FRAMES):
        since = f - R.RESET_FRAME
        want_valid = [] if f < max_delay else (others if 0 <= since < max_delay else everyone)
        assert valid[f] == want_valid, (f, valid[f])
        assert (got[f] is None) == (f < max_delay) and (scalar[f] is None) == (f < max_delay)
        if got[f] is None:
            continue
        for b in others:
            assert torch.equal(got[f][b], scalar[f][b]), (f, b)
            assert torch.equal(got[f][b:b + 1], runs[(b, 0)][f]), (f, b)
        b = R.RESET_ROW
        if f < R.RESET_FRAME:
            assert torch.equal(got[f][b], scalar[f][b]) and torch.equal(got[f][b:b + 1], runs[(b, 0)][f]), f
        elif since >= max_delay:
            assert torch.equal(got[f][b:b + 1], runs[(b, R.RESET_FRAME)][since]), (f, got[f][b].flatten().tolist())
    if graphs:
        with gen.streaming(R.B, per_stream=True), torch.no_grad():
            g0 = gen._streaming_state.graphed_frame
            for f in range(4):
                if f == 3:
                    gen.reset_streams([0])
                gen.step(user[f].to(DEV))
            assert gen._streaming_state.graphed_frame is g0 and g0.graph is not None and g0.calls == 2, "a reset must not re-capture the frame"
            assert gen._streaming_state.offset_dev.tolist() == [1, 4, 4] and gen.lm_model.transformer._streaming_state.pos.tolist() == [1, 4, 4]


# ------------------------------------------------------------------------------------------------------------ 6: the pipeline

PIPE_B, PIPE_FRAMES, PIPE_ROW, PIPE_AT = 3, 9, 1, 5


@functools.lru_cache(maxsize=1)
def _pipe_models():
    cfg = dict(synth.LM_TINY_16Q)
    lm_sd = synth.lm_state_dict(cfg, seed=9)
    model = LMModel.from_state_dict({k: v.to(DEV) for k, v in lm_sd.items()}, cfg)
    return cfg, lm_sd, LMGen(model, use_sampling=False)


def _pipe_run(pcm, frames, client_rate, per_stream, reset_at=None):
    """-> (list of PCM per frame (None inside the session's delay), valid rows per frame, (fused graph before the restart, after))."""
    _, mimi = _mimi()
    _, _, gen = _pipe_models()
    outs, valid, graphs = [], [], [None, None]
    with StreamingPipeline(mimi, gen, PIPE_B, client_rate=client_rate, per_stream=per_stream) as pipe:
        n = pipe.client_frame
        for f in frames:
            if f == reset_at:
                graphs[0] = (pipe._fused, pipe._fused.graph, pipe._fused.calls) if pipe._fused is not None else None
                pipe.reset_streams([PIPE_ROW])
            o = pipe.step(pcm[:, :, f * n:(f + 1) * n].contiguous().to(DEV))
            outs.append(None if o is None else o.cpu())
            valid.append(list(pipe.stream_valid) if per_stream else None)
        graphs[1] = (pipe._fused, pipe._fused.graph, pipe._fused.calls) if pipe._fused is not None else None
    return outs, valid, graphs


@pytest.mark.parametrize("client_rate", [None, 48000], ids=["24k", "48k"])
def test_pipeline_restart(client_rate):
    cfg, lm_sd, gen = _pipe_models()
    mimi_sd, _ = _mimi()
    max_delay = gen.max_delay
    n = FRAME if client_rate is None else FRAME * client_rate // 24000
    pcm = synth.synth_audio(PIPE_B, PIPE_FRAMES * n, seed=21)
    frames = range(PIPE_FRAMES)
    plain, valid0, _ = _pipe_run(pcm, frames, client_rate, per_stream=True)
    if client_rate is None:
        scalar, _, _ = _pipe_run(pcm, frames, client_rate, per_stream=False)
        for f in frames:
            assert (plain[f] is None) == (scalar[f] is None) == (f < max_delay)
            assert plain[f] is None or torch.equal(plain[f], scalar[f]), f
    assert valid0 == [[] if f < max_delay else [0, 1, 2] for f in frames]
    got, valid, graphs = _pipe_run(pcm, frames, client_rate, per_stream=True, reset_at=PIPE_AT)
    # one frame graph, captured before the restart, replayed before and after it
    assert graphs[0] is not None and graphs[0][1] is not None, "the frame was not yet one graph when the row restarted"
    assert graphs[1][0] is graphs[0][0] and graphs[1][1] is graphs[0][1] and graphs[1][2] == graphs[0][2], "the restart re-captured the frame"
    new, _, _ = _pipe_run(pcm, range(PIPE_AT, PIPE_FRAMES), client_rate, per_stream=True)
    others = [b for b in range(PIPE_B) if b != PIPE_ROW]
    for f in frames:
        since = f - PIPE_AT
        if f < max_delay:
            assert got[f] is None and valid[f] == []
            continue
        assert valid[f] == (others if 0 <= since < max_delay else [0, 1, 2]), (f, valid[f])
        assert torch.equal(got[f][others], plain[f][others]), f
        if since < 0:
            assert torch.equal(got[f][PIPE_ROW], plain[f][PIPE_ROW]), f
        elif since < max_delay:
            assert float(got[f][PIPE_ROW].abs().max()) == 0.0, f
        else:
            assert torch.equal(got[f][PIPE_ROW], new[since][PIPE_ROW]), f
    assert not torch.equal(got[-1][PIPE_ROW], plain[-1][PIPE_ROW]), "the restart changed nothing: the test shows nothing"
    if client_rate is None:
        # the restarted conversation against the composed oracles (the bound of tests/test_e2e_gpu.py)
        mcfg = O.MimiConfig()
        mine = pcm[PIPE_ROW:PIPE_ROW + 1, :, PIPE_AT * FRAME:]
        with torch.no_grad():
            codes = O.encode(mimi_sd, mcfg, mine)
            og = L.LMGenOracle({k: v.float() for k, v in lm_sd.items()}, L.LMConfig(**cfg), 1)
            toks = [og.step(codes[:, :, f:f + 1]) for f in range(PIPE_FRAMES - PIPE_AT)]
            ref = O.decode(mimi_sd, mcfg, torch.cat([t[:, 1:] for t in toks[max_delay:]], -1))
        mine_out = torch.cat([got[f][PIPE_ROW:PIPE_ROW + 1] for f in range(PIPE_AT + max_delay, PIPE_FRAMES)], -1)
        assert mine_out.shape == ref.shape
        err = float((mine_out - ref).abs().max() / ref.abs().max())
        print(f"restarted row vs the composed oracles: rel err {err:.3e}")
        assert err < 1e-3, err


def test_pipeline_reset_needs_the_mode():
    _, mimi = _mimi()
    _, _, gen = _pipe_models()
    with StreamingPipeline(mimi, gen, PIPE_B) as pipe:
        with pytest.raises(ValueError, match="per_stream=True"):
            pipe.reset_streams([0])
    with StreamingPipeline(mimi, gen, PIPE_B, per_stream=True) as pipe:
        with pytest.raises(ValueError, match="outside the batch"):
            pipe.reset_streams([PIPE_B])
