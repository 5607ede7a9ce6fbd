"""Per-stream sampling on the GPU.  Scenarios, seeds and the numpy noise: tests/helpers/stream_sampling.py; the margins
the token equalities rest on: tests/test_stream_sampling_cpu.py.

1. ``ops.noise_exp_rows`` (rst_noise_exp_ps_f32) against the fp64 ``-log u`` of the exact uniform, within 4 ulp (the scaling is exact,
   OpenCL bounds ``log`` at 3 ulp, rounding the reference adds at most 1); tails, padding and a guard row untouched; repeatable.
2. ``ops.lm_sample_ps`` (rst_lm_sample_ps_f32) row by row against ``oracle.lm_oracle.sample_token``: greedy, top-1, the cap and
   in between in one launch, every instantiation of the one-level kernel, per-row id limits, the clamp, the NULL-table front.
3. ``LMGen(per_stream_sampling=True)``: a stream == the same conversation alone == among other neighbours == the oracle fed the launch's
   noise; a reset stream with its seed replays itself; a change of settings changes one stream from that frame on; one graph throughout.
4. The slot server with ``sampling=`` per client: every conversation == a new pipeline's with that client's settings and seed.
5. Refusals."""
import functools

import numpy as np
import pytest
import torch

from oracle import lm_oracle as L
from rstnet_amd import _lib, ops, synth
from rstnet_amd import server as S
from rstnet_amd.codec.loaders import get_mimi
from rstnet_amd.lm.model import LMGen, LMModel
from rstnet_amd.pipeline import StreamingPipeline
from tests.helpers import slot_server as SS
from tests.helpers import stream_sampling as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = -7.0


def _seed_tensor(seeds) -> torch.Tensor:
    """uint64 seeds as the int64 tensor the library reads them from."""
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64, device=DEV)


def _device_noise(seed: int, frame: int, n_cols: int) -> torch.Tensor:
    return ops.noise_exp_rows(_seed_tensor([seed]), torch.tensor([frame], dtype=torch.int64, device=DEV), n_cols)[0].cpu()


# ------------------------------------------------------------------------------------------------------------------------ 1: the noise

NOISE_SEEDS, NOISE_FRAMES = (0, 1, 2 ** 63 + 5), (0, 1, 2 ** 32 + 7)


@pytest.mark.parametrize("frame_stride", [1, 0], ids=["per-stream", "shared"])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n_cols", [1, 3, 4, 5, 2025])
def test_noise_launch(n_cols, pad, frame_stride):
    Bn = len(NOISE_SEEDS)
    seeds = _seed_tensor(NOISE_SEEDS)
    frames = torch.tensor(NOISE_FRAMES if frame_stride else NOISE_FRAMES[2:], dtype=torch.int64, device=DEV)
    buf = torch.full((Bn + 1, n_cols + pad), GUARD, device=DEV)
    got = ops.noise_exp_rows(seeds, frames, n_cols, out=buf[:Bn])
    assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (Bn, n_cols)
    host = buf.cpu().numpy()
    assert (host[Bn] == GUARD).all() and (host[:Bn, n_cols:] == GUARD).all(), "the launch wrote past a row's n_cols columns"
    worst = 0.0
    for b in range(Bn):
        want = H.noise_f64(NOISE_SEEDS[b], NOISE_FRAMES[b] if frame_stride else NOISE_FRAMES[2], n_cols)
        assert np.isfinite(host[b, :n_cols]).all() and (host[b, :n_cols] > 0).all()
        worst = max(worst, float(H.ulp_distance(host[b, :n_cols], want).max()))
    print(f"n_cols {n_cols}, stride {n_cols + pad}, frame_stride {frame_stride}: {worst:.2f} ulp from -log(u) in fp64")
    assert worst <= 4.0
    again = ops.noise_exp_rows(seeds, frames, n_cols)
    assert again.is_contiguous() and torch.equal(again.view(torch.int32), got.view(torch.int32)), "equal arguments, other bits"


# -------------------------------------------------------------------------------------------------------------- 2: the per-row sampler

def _sampler_inputs(V: int):
    cap, rows = H.sampler_cap(V), H.sampler_rows(V)
    logits = H.sampler_logits(V).to(DEV)
    noise = ops.noise_exp_rows(_seed_tensor(H.SAMPLER_SEEDS), torch.tensor([H.SAMPLER_FRAME], dtype=torch.int64, device=DEV), cap)
    temps = torch.tensor([t for t, _ in rows], dtype=torch.float32, device=DEV)
    top_ks = torch.tensor([k for _, k in rows], dtype=torch.int32, device=DEV)
    return cap, logits, noise, temps, top_ks


@pytest.mark.parametrize("V", H.SAMPLER_V)
def test_sampler_rows_against_the_oracle(V):
    cap, logits, noise, temps, top_ks = _sampler_inputs(V)
    want, _ = H.sampler_reference(V, limits=False)
    got = ops.lm_sample_ps(logits, top_k=cap, noise=noise, temps=temps, top_ks=top_ks)
    assert got.tolist() == want
    # the oracle fed what the launch wrote (not the numpy noise) says the same
    host = noise.cpu()
    for b, (t, k) in enumerate(H.sampler_rows(V)):
        assert int(L.sample_token(H.sampler_logits(V)[b][None], t > 0.0, t, k, host[b, :k][None])[0]) == want[b]
    # per-row id limits on top (the greedy row ignores its limit, as the scalar sampler does)
    want_l, _ = H.sampler_reference(V, limits=True)
    limits = torch.tensor(H.sampler_limits(V), dtype=torch.int32, device=DEV)
    got_l = ops.lm_sample_ps(logits, top_k=cap, noise=noise, temps=temps, top_ks=top_ks, limit_dev=limits)
    assert got_l.tolist() == want_l and want_l != want
    # the clamp: a table entry of 0 behaves as 1, one of cap + 9 as the cap (rows 1 and 2 hold exactly 1 and the cap above)
    bad = top_ks.clone()
    bad[1], bad[2] = 0, cap + 9
    assert ops.lm_sample_ps(logits, top_k=cap, noise=noise, temps=temps, top_ks=bad).tolist() == want
    # strided tables (two columns of [B, 3] tables) and a column of a wider token buffer
    t3, k3 = torch.zeros(4, 3, device=DEV), torch.zeros(4, 3, dtype=torch.int32, device=DEV)
    t3[:, 1], k3[:, 1] = temps, top_ks
    out = torch.full((4, 2), -1, dtype=torch.int64, device=DEV)
    ops.lm_sample_ps(logits, top_k=cap, noise=noise, temps=t3[:, 1], top_ks=k3[:, 1], out=out[:, 1])
    assert out[:, 1].tolist() == want and out[:, 0].tolist() == [-1] * 4


@pytest.mark.parametrize("V", H.SAMPLER_V)
def test_null_tables_are_the_rows_entry_point(V):
    cap, logits, noise, _, _ = _sampler_inputs(V)
    lib = _lib.lib()
    limits = torch.tensor(H.sampler_limits(V), dtype=torch.int32, device=DEV)
    for use_sampling, temp, k in ((1, 0.8, 7), (1, 1.0, cap), (0, 0.8, 7)):
        a, b = torch.full((4,), -1, dtype=torch.int64, device=DEV), torch.full((4,), -1, dtype=torch.int64, device=DEV)
        args = (logits.data_ptr(), noise.data_ptr(), None, 4, V, V, k, noise.stride(0), 1, use_sampling, temp, 0, limits.data_ptr(), 1, 0.0, None, 0,
                torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.rst_lm_sample_rows_f32(args[0], args[1], a.data_ptr(), *args[3:]))
        _lib.check(lib.rst_lm_sample_ps_f32(args[0], args[1], b.data_ptr(), *args[3:], None, None, 0))
        assert torch.equal(a, b) and int(a.min()) >= 0


# ---------------------------------------------------------------------------------------------------------------------------- 3: LMGen

@functools.lru_cache(maxsize=1)
def _tiny_lm():
    return LMModel.from_state_dict({k: v.to(DEV) for k, v in H.lm_state().items()}, H.CFG)


def _session(settings, user, events=None):
    """One per-stream session of ``len(settings)`` streams with graphs on: ``settings[b]`` applied before frame 0, ``events[f](gen, f)``
    before frame ``f``.  -> (per frame ``None`` or int64 ``[B, dep_q + 1]`` on the host, the frame's (Graphed, graph, calls) after the
    first replayed frame and after the last one)."""
    n = len(settings)
    gen = LMGen(_tiny_lm(), top_k=H.TOP_K_CAP, top_k_text=H.TOP_K_TEXT_CAP, per_stream_sampling=True)
    outs, marks = [], []
    with gen.streaming(n, per_stream=True), torch.no_grad():
        for b, s in enumerate(settings):
            gen.set_stream_sampling([b], **s)
            assert gen.stream_sampling(b) == s
        for f in range(user.shape[0]):
            if events and f in events:
                events[f](gen)
            o = gen.step(user[f].to(DEV))
            outs.append(None if o is None else o[:, :, 0].cpu())
            if f in (1, user.shape[0] - 1):
                g = gen._streaming_state.graphed_frame
                marks.append((g, g.graph, g.calls))
    return outs, marks


def _row(outs, b, frames, d=max(H.CFG["delays"])):
    """Stream ``b``'s outputs at session frames ``frames`` -- its own frames 0, 1, ... -- from its first meaningful one on."""
    return [outs[f][b] for f in list(frames)[d:]]


@functools.lru_cache(maxsize=1)
def _main():
    return _session(H.ROWS, H.user_tokens())


def _same(a, b) -> bool:
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("b", range(H.B))
def test_lmgen_stream_equals_itself_alone_and_among_others(b):
    main, _ = _main()
    user = H.user_tokens()
    every = range(H.FRAMES)
    assert all(o is None for o in main[:1]) and all(o is not None for o in main[1:])
    # (a) alone: a session of one stream with this stream's settings, seed and user tokens
    alone, _ = _session([H.ROWS[b]], user[:, b:b + 1])
    assert _same(_row(main, b, every), _row(alone, 0, every)), f"stream {b} alone says something else"
    # (b) among others: the neighbours have other tokens, settings and seeds
    other_user = H.user_tokens(seed=H.USER_SEED + 1)
    other_user[:, b] = user[:, b]
    settings = [H.ROWS[b] if r == b else dict(H.OTHER, seed=H.OTHER["seed"] + r) for r in range(H.B)]
    among, _ = _session(settings, other_user)
    assert _same(_row(main, b, every), _row(among, b, every)), f"stream {b} depends on its neighbours"
    others = [r for r in range(H.B) if r != b]
    assert not all(_same(_row(main, r, every), _row(among, r, every)) for r in others), "the other neighbours said the same: vacuous"


@pytest.mark.parametrize("b", range(H.B))
def test_lmgen_stream_equals_the_oracle_fed_the_launchs_noise(b):
    main, _ = _main()
    runs, margin, _ = H.lmgen_oracle_runs()
    assert margin >= H.MARGIN
    sd = {k: v.float() for k, v in H.lm_state().items()}
    with torch.no_grad():
        ref = H.oracle_conversation(sd, H.CFG, H.user_tokens()[:, b:b + 1], H.ROWS[b], (H.TOP_K_CAP, H.TOP_K_TEXT_CAP), noise_fn=_device_noise)
    for f in range(H.FRAMES):
        assert (ref[f] is None) == (runs[b][f] is None) and (ref[f] is None or torch.equal(ref[f], runs[b][f])), "numpy noise and the launch's disagree"
        if ref[f] is not None:
            assert torch.equal(main[f][b], ref[f][0, :, 0]), f"stream {b}, frame {f}: {main[f][b].tolist()} against the oracle's {ref[f][0, :, 0].tolist()}"


def test_lmgen_reset_replays_and_a_change_of_settings_stays_in_its_row():
    main, main_marks = _main()
    user = H.user_tokens().clone()
    R, F0, W, F1 = H.RESET_ROW, H.RESET_FRAME, H.SWITCH_ROW, H.SWITCH_FRAME
    replay = H.FRAMES - F0
    user[F0:, R] = H.user_tokens()[:replay, R]     # the restarted stream hears its first frames again (source and target overlap: not in place)

    def restart(gen):
        gen.reset_streams([R])
        assert gen.stream_sampling(R)["seed"] != H.ROWS[R]["seed"], "a reset draws a new seed"
        gen.set_stream_sampling([R], seed=H.ROWS[R]["seed"])
        assert gen.stream_sampling(R) == H.ROWS[R]

    def switch(gen):
        gen.set_stream_sampling([W], **H.SWITCH)
        assert gen.stream_sampling(W) == dict(H.ROWS[W], **H.SWITCH)

    outs, marks = _session(H.ROWS, user, {F0: restart, F1: switch})
    every = range(H.FRAMES)
    # (d) the restarted stream repeats its frames 0 .. 7; the others go on undisturbed
    assert _same(_row(outs, R, range(F0, H.FRAMES)), _row(main, R, range(replay)))
    assert _same(_row(outs, R, range(F0)), _row(main, R, range(F0)))
    assert _same(_row(outs, 0, every), _row(main, 0, every))
    # (e) the changed stream: as before up to the change, then as a session (alone) that changed at the same frame, and as the oracle
    assert _same(_row(outs, W, range(F1)), _row(main, W, range(F1)))
    alone, _ = _session([H.ROWS[W]], H.user_tokens()[:, W:W + 1], {F1: lambda gen: gen.set_stream_sampling([0], **H.SWITCH)})
    assert _same(_row(outs, W, every), _row(alone, 0, every))
    runs, _, _ = H.lmgen_oracle_runs()
    assert _same(_row(outs, W, every), [r[0, :, 0] for r in runs["switch"][1:]])
    assert not _same(_row(outs, W, every), _row(main, W, every)), "the new settings changed nothing: vacuous"
    # (f) one graph: the object, its capture and its call count after the last frame are those after the first replayed one
    for (g0, graph0, calls0), (g1, graph1, calls1) in (marks, main_marks):
        assert g0 is g1 and graph0 is graph1 and graph0 is not None and calls0 == calls1 == 2


# ------------------------------------------------------------------------------------------------------------------ 4: the slot server

FRAME = SS.FRAME


@functools.lru_cache(maxsize=1)
def _models():
    mimi = get_mimi(synth.mimi_state_dict(H.SLOT_MIMI_SEED), device=DEV)
    lm = LMModel.from_state_dict({k: v.to(DEV) for k, v in synth.lm_state_dict(SS.cfg(), seed=H.SLOT_LM_SEED).items()}, SS.cfg())
    return mimi, lm


def _messages(state_like, fmt: str, wav_row: np.ndarray, token: int):
    msgs = [(S.KIND_AUDIO, S.PcmFramer(FRAME, fmt).encode(wav_row))]
    piece = state_like.text_piece(token)
    if piece is not None:
        msgs.append((S.KIND_TEXT, piece.encode("utf8")))
    return msgs


def _reference(st, name: str, neighbour_seed: int):
    """Client ``name``'s conversation in its row of a NEW per-stream pipeline, from frame 0, with its settings and seed; the other rows
    hear other audio and sample by other settings and seeds."""
    mimi, lm = _models()
    row, fmt = SS.CLIENTS[name][0], SS.CLIENTS[name][1]
    audio = SS.heard(name)
    n = audio.shape[-1] // FRAME
    pcm = synth.synth_audio(SS.N, n * FRAME, seed=neighbour_seed)
    pcm[row] = audio[0]
    out = []
    with StreamingPipeline(mimi, LMGen(lm, per_stream_sampling=True), SS.N, per_stream=True) as pipe:
        for r in range(SS.N):
            if r == row:
                pipe.set_stream_sampling([r], **H.SLOT_SAMPLING[name])
            else:
                pipe.set_stream_sampling([r], temp=1.2, temp_text=1.1, top_k=3 + r, top_k_text=2 + r, seed=neighbour_seed + r)
        assert pipe.stream_sampling(row) == H.slot_settings(name)
        for f in range(n):
            wav = pipe.step(pcm[:, :, f * FRAME:(f + 1) * FRAME].contiguous().to(DEV))
            if wav is None or row not in pipe.stream_valid:
                out.append([])
                continue
            out.append(_messages(st, fmt, wav[row, 0].cpu().numpy(), int(pipe.last_tokens[row, 0])))
    return out


def test_slot_server_conversations_equal_new_sessions_with_their_settings():
    mimi, lm = _models()
    st = S.SlotServerState(mimi, lm, DEV, slots=SS.N, per_slot_sampling=True)
    try:
        pipe = st.pipe
        st.warmup()
        fused = (pipe._fused, pipe._fused.graph, pipe._fused.calls)
        assert fused[1] is not None, "the served frame is not one graph after warm-up"
        slot, got = {}, {name: [] for name in SS.CLIENTS}
        with torch.no_grad():
            for tick in range(SS.TICKS):
                for name, (row, fmt, t0, t1, _, _) in SS.CLIENTS.items():
                    if tick == t1 and name in slot:
                        st.leave(slot.pop(name))
                for name, (row, fmt, t0, t1, _, _) in SS.CLIENTS.items():
                    if tick == t0:
                        slot[name] = st.join(fmt, sampling=H.SLOT_SAMPLING[name])
                        assert slot[name] == row, (name, slot[name])
                for name, s in slot.items():
                    p = SS.payloads(name)[tick - SS.CLIENTS[name][2]]
                    if p is not None:
                        st.push(s, p)
                out = st.tick()
                for name, s in slot.items():
                    assert pipe.stream_sampling(s) == H.slot_settings(name)
                    got[name].append(out.get(s, []))
        assert pipe._fused is fused[0] and pipe._fused.graph is fused[1] and pipe._fused.calls == fused[2], "joins with settings re-captured the frame"
        assert {k: v for k, v in pipe.stream_sampling(2).items() if k != "seed"} == pipe.lm_gen.default_sampling(), "the free row lost the defaults"
    finally:
        st.close()

    d = st.max_delay
    for i, name in enumerate(SS.CLIENTS):
        row, fmt, t0, t1, _, _ = SS.CLIENTS[name]
        want = _reference(st, name, neighbour_seed=170 + 10 * i)
        assert len(got[name]) == len(want) == t1 - t0
        assert all(m == [] for m in got[name][:d]) and all(len(m) >= 1 for m in got[name][d:]), name
        for f, (a, b) in enumerate(zip(got[name], want)):
            assert a == b, f"client {name}, frame {f}: {[(k, len(p)) for k, p in a]} against {[(k, len(p)) for k, p in b]}"


# ------------------------------------------------------------------------------------------------------------------------ 5: refusals

def test_refusals_launch_nothing():
    lm = _tiny_lm()
    user = H.user_tokens()
    plain = LMGen(lm, top_k=H.TOP_K_CAP, top_k_text=H.TOP_K_TEXT_CAP)
    with plain.streaming(2, per_stream=True):
        with pytest.raises(ValueError, match="per_stream_sampling=True"):
            plain.set_stream_sampling([0], temp=0.5)
        with pytest.raises(ValueError, match="per_stream_sampling=True"):
            plain.stream_sampling(0)
    gen = LMGen(lm, top_k=H.TOP_K_CAP, top_k_text=H.TOP_K_TEXT_CAP, per_stream_sampling=True)
    with gen.streaming(2):                                     # a scalar session of such an LMGen has no tables either
        with pytest.raises(ValueError, match="per_stream=True"):
            gen.set_stream_sampling([0], temp=0.5)
    with gen.streaming(2, per_stream=True):
        before = [gen.stream_sampling(b) for b in range(2)]
        tables = gen._streaming_state.sampling
        snap = [t.clone() for t in (tables.temp, tables.temp_text, tables.top_k, tables.top_k_text, tables.seed)]
        for kw, why in ((dict(top_k=H.TOP_K_CAP + 1), r"1 \.\. 8"), (dict(top_k_text=0), r"1 \.\. 10"), (dict(temp=-1.0), "temperature"),
                        (dict(temp=0.5, temp_text=float("nan")), "temperature"), (dict(seed=[1]), "values for 2 rows"), (dict(seed=-1), "seed")):
            with pytest.raises(ValueError, match=why):
                gen.set_stream_sampling([0, 1], **kw)
        with pytest.raises(ValueError, match="outside the batch"):
            gen.set_stream_sampling([2], temp=0.5)
        assert [gen.stream_sampling(b) for b in range(2)] == before, "a refused call changed the host mirror"
        now = (tables.temp, tables.temp_text, tables.top_k, tables.top_k_text, tables.seed)
        assert all(torch.equal(a, b) for a, b in zip(snap, now)), "a refused call wrote a table"
        gen.set_stream_sampling([1], use_sampling=False)
        assert tables.temp.tolist()[1] == 0.0 and tables.temp_text.tolist()[1] == 0.0 and gen.stream_sampling(1)["temp"] == before[1]["temp"]
        gen.set_stream_sampling([1], use_sampling=True)
        assert gen.stream_sampling(1) == before[1] and torch.equal(tables.temp, snap[0]) and torch.equal(tables.temp_text, snap[1])
    with pytest.raises(ValueError):
        LMGen(lm, top_k=0, per_stream_sampling=True)           # "all ids" is no cap
    # the sampler: per-row tables with top_p, above the one-level kernel's vocabularies, through ops and through the library
    temps, top_ks = torch.full((2,), 0.8, device=DEV), torch.full((2,), 3, dtype=torch.int32, device=DEV)
    noise = torch.ones(2, 50, device=DEV)
    out = torch.full((2,), -5, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="top_p"):
        ops.lm_sample_ps(torch.zeros(2, 50, device=DEV), top_k=5, noise=noise, top_p=0.9, temps=temps, top_ks=top_ks, out=out)
    big = torch.zeros(2, 151936, device=DEV)
    with pytest.raises(ValueError, match="32768"):
        ops.lm_sample_ps(big, top_k=5, noise=noise, temps=temps, top_ks=top_ks, out=out)
    with pytest.raises(ValueError, match="pair"):
        ops.lm_sample_ps(torch.zeros(2, 50, device=DEV), top_k=5, noise=noise, temps=temps, top_ks=None, out=out)
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    for V, logits, top_p, ws in ((50, noise, 0.9, big), (151936, big, 0.0, None)):
        rc = lib.rst_lm_sample_ps_f32(logits.data_ptr(), noise.data_ptr(), out.data_ptr(), 2, V, V, 5, 50, 1, 1, 1.0, 0, None, 0, top_p,
                                      None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, stream,
                                      temps.data_ptr(), top_ks.data_ptr(), 1)
        assert rc != 0 and b"per-row parameters" in lib.rst_last_error()
    # the noise launch: B <= 0, n_cols <= 0, a stride below n_cols, a NULL pointer
    seeds, frames = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    nbuf = torch.full((2, 8), GUARD, device=DEV)
    for args in ((nbuf.data_ptr(), 0, 8, 8, seeds.data_ptr(), frames.data_ptr()), (nbuf.data_ptr(), 2, 0, 8, seeds.data_ptr(), frames.data_ptr()),
                 (nbuf.data_ptr(), 2, 8, 7, seeds.data_ptr(), frames.data_ptr()), (None, 2, 8, 8, seeds.data_ptr(), frames.data_ptr()),
                 (nbuf.data_ptr(), 2, 8, 8, None, frames.data_ptr()), (nbuf.data_ptr(), 2, 8, 8, seeds.data_ptr(), None)):
        assert lib.rst_noise_exp_ps_f32(*args, 1, stream) != 0 and b"noise_exp" in lib.rst_last_error()
    torch.cuda.synchronize()
    assert out.tolist() == [-5, -5] and (nbuf == GUARD).all(), "a refused call launched"
    del user
