"""The streamed Mimi step at more than two streams (the codec share of a many-stream server frame), at the stream counts S where
its routes change, against fp64 and against the fixtures:

  S = 3   smallest count on the layer loop (B <= 2 runs both transformers as the persistent `codec_tr` launch)
  S = 9   the 6 kHz k8 s4 convolution has 4320 > 4096 rows: 128 x 128 tiles, fewer than the CUs -> the 32-row tiles, with a history
  S = 32  a 32-stream server frame
  S = 64  the 25 Hz linears have 2S = SKINNY_F32_MAX_ROWS = 128 rows, the last count on the few-row route
  S = 65  130 rows: the 25 Hz linears leave the few-row route (kernel level only)

(the tests assert these crossings from the recorded launches and the library's own plans; the table is only the map).

1. Whole Mimi, 150 frames (the 250-slot rings of both transformers wrap at frame 125), the two clips of mimi_stream_long.npz in
   slots 0 and S - 1 and other audio elsewhere: fixture parity of those two slots, eager == graph-replayed codes, one clipped
   stream against the CPU oracle's streamed path.
2. Stream isolation: the same session with every other slot's audio and codes replaced gives bit-identical codes and waveforms
   in the fixture slots (no kernel of this route reduces across rows).
3. Every GEMM-like call of one eager streamed frame, replayed with random operands and a random non-zero history per stream at
   its real sizes, against fp64 with per-element bounds; the one-launch attention step against an fp64 ring attention.
4. The routes part 3 relies on, asserted from ops.PROFILE of a real frame.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mimi_oracle as O
from rstnet_amd import _lib, ops, synth
from rstnet_amd.codec import functional as RF
from rstnet_amd.codec.mimi import MimiCodec
from tests.golden import cases
from tests.helpers import codec_streams as CS
from tests.parity import codes_match_up_to_near_ties

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
U = CS.U
FRAME = CS.FRAME
# Backward-error constant of the f32 GEMM routes: |y - ref| <= C_GEMM * 2^-24 * (sum_k |x_k| |w_k| + |bias|) (+ the epilogue's own
# terms, CS.epilogue64) -- the form and constant of test_gemm_b3_gpu.py, set there against a measured 5.3 - 6.1 for the f32 instruction.
C_GEMM = 16.0


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@functools.lru_cache(maxsize=1)
def _mimi():
    sd = synth.mimi_state_dict(cases.MIMI_SEED, layer_scale=cases.TRANSFORMER_LAYER_SCALE)
    return sd, MimiCodec.from_state_dict(sd).to(DEV)


def _card(sd) -> int:
    return sd["quantizer.rvq_first.vq.layers.0._codebook.embedding_sum"].shape[0]


# ------------------------------------------------------------------------------------------------------------ 1 + 2: model level

LONG = cases.MIMI_STREAM_LONG          # (2 streams, 150 frames, seed)


def _streams(S: int, variant: int):
    """Audio [S, 1, 150 frames] and decode codes [S, 8, 150]: the fixture's clips / codes in slots 0 and S - 1, a full-scale
    clipped stream in slot 1 (its decode slot gets the oracle's codes of that clip), a near-silent stream in slot 2 (S > 3), other
    seeded audio and random valid codes elsewhere.  `variant` re-seeds every non-fixture slot (and swaps the clipped / near-silent
    ones for other audio), keeping the fixture slots as they are."""
    _, frames, seed = LONG
    sd, _ = _mimi()
    fix = synth.synth_audio(2, FRAME * frames, seed=seed)
    g = torch.Generator().manual_seed(500 + 31 * S + 1000 * variant)
    audio = 0.1 * torch.randn(S, 1, FRAME * frames, generator=g) * (0.5 + torch.rand(S, 1, 1, generator=g))
    codes = torch.randint(0, _card(sd), (S, 8, frames), generator=g)
    ref_codes = torch.from_numpy(np.load(os.path.join(G, "mimi_stream_long.npz"))["codes"]).long()
    audio[0], audio[S - 1] = fix[0], fix[1]
    codes[0], codes[S - 1] = ref_codes[0], ref_codes[1]
    if variant == 0:
        audio[1] = _clipped()
        codes[1] = _clipped_oracle()[0][0]
        if S > 3:
            audio[2] = 1e-4 * synth.synth_audio(1, FRAME * frames, seed=91)[0]
    return audio, codes


@functools.lru_cache(maxsize=1)
def _clipped() -> torch.Tensor:
    """[1, T]: a full-scale stream, clipped (8x the synthetic level, clamped to +-1)."""
    return (8 * synth.synth_audio(1, FRAME * LONG[1], seed=90)[0]).clamp(-1.0, 1.0)


def _oracle_gaps(sd, z, B):
    """Top-2 relative gap of every RVQ decision of the oracle for latent `z` (as make_golden.py records it for the fixtures)."""
    gaps = []
    for p, n_q in (("quantizer.rvq_first", 1), ("quantizer.rvq_rest", 7)):
        r = F.conv1d(z, sd[f"{p}.input_proj.weight"]).transpose(1, 2).reshape(-1, 256)
        for j in range(n_q):
            emb = O.codebook(sd, f"{p}.vq.layers.{j}")
            t2 = torch.cdist(r[None], emb[None])[0].topk(2, largest=False)
            gaps.append(((t2.values[:, 1] - t2.values[:, 0]) / t2.values[:, 0]).view(B, -1))
            r = r - emb[t2.indices[:, 0]]
    return torch.stack(gaps, 1)


@functools.lru_cache(maxsize=1)
def _clipped_oracle():
    """The CPU oracle's streamed path on the clipped stream alone (streams are independent): (codes [1, 8, F], gaps, waveform of
    those codes)."""
    sd, _ = _mimi()
    cfg = O.MimiConfig()
    with torch.no_grad():
        z = O.encode_latent_streamed(sd, cfg, _clipped()[None])
        codes = O.rvq_encode(sd, cfg, z)
        gaps = _oracle_gaps(sd, z, 1)
        wav = O.decode_streamed(sd, cfg, codes)
    return codes, gaps, wav


def _session(S: int, variant: int, eager: bool):
    """150 frames of S streams: (eager codes or None, latent [S, 512, F] or None, graph-replayed codes, waveform of the decode
    codes), all on the CPU."""
    _, model = _mimi()
    audio, dcodes = _streams(S, variant)
    frames = LONG[1]
    audio, dcodes = audio.to(DEV), dcodes.to(DEV)
    cs_eager = zs = None
    if eager:
        zs, cs_eager = [], []
        with model.streaming(S), torch.no_grad():
            for f in range(frames):
                z = model.encode_latent(audio[:, :, f * FRAME:(f + 1) * FRAME].contiguous())
                zs.append(z)
                cs_eager.append(model.quantizer.encode_nlc(z))
        zs = torch.cat(zs, 1).transpose(1, 2).cpu()
        cs_eager = torch.cat(cs_eager, -1).cpu()
    cs, ws = [], []
    with model.streaming(S):
        for f in range(frames):
            cs.append(model.encode(audio[:, :, f * FRAME:(f + 1) * FRAME].contiguous()))
            ws.append(model.decode(dcodes[:, :, f:f + 1].contiguous()))
    torch.cuda.synchronize()
    assert ops.codec_transformer_status(torch.device(DEV)).tolist()[:3] == [0, 0, 0], "a persistent transformer launch timed out"
    return cs_eager, zs, torch.cat(cs, -1).cpu(), torch.cat(ws, -1).cpu()


_sessions: dict = {}


def _cached_session(S: int, variant: int, eager: bool):
    key = (S, variant)
    if key not in _sessions or (eager and _sessions[key][0] is None):
        if len(_sessions) > 2:
            _sessions.clear()
        _sessions[key] = _session(S, variant, eager)
    return _sessions[key]


@pytest.mark.parametrize("S", [3, 9, 32, 64])
def test_many_streams_past_the_wrap_match_fixture_and_oracle(S):
    """150 frames at S streams (the layer loop with the one-launch attention step, never `codec_tr`): the fixture's two clips in slots
    0 / S - 1 meet mimi_stream_long.npz as test_mimi_long_stream_matches_moshi_fixture does at B = 2; eager frames == graph-replayed
    frames; the clipped stream in slot 1 against the oracle's streamed path; the persistent launches' status stays clean."""
    sd, _ = _mimi()
    g = np.load(os.path.join(G, "mimi_stream_long.npz"))
    tail = cases.MIMI_STREAM_LONG_TAIL
    cs_eager, z, codes, wav = _cached_session(S, 0, eager=True)
    assert torch.equal(codes, cs_eager), f"S={S}: graph-replayed frames differ from eager frames"
    fx = [0, S - 1]
    ref_codes = torch.from_numpy(g["codes"]).long()
    excused = codes_match_up_to_near_ties(codes[fx], ref_codes, torch.from_numpy(g["rel_gap"]))
    n_near = int((g["rel_gap"] < 2e-5).sum())
    e_lat = rel_err(z[fx][:, :, -tail:], torch.from_numpy(g["latent_tail"]))
    e_head = rel_err(wav[fx][:, :, :FRAME * 4], torch.from_numpy(g["wav_head"]))
    e_tail = rel_err(wav[fx][:, :, -FRAME * tail:], torch.from_numpy(g["wav_tail"]))
    o_codes, o_gaps, o_wav = _clipped_oracle()
    o_excused = codes_match_up_to_near_ties(codes[1:2], o_codes, o_gaps)
    e_clip = rel_err(wav[1:2], o_wav)
    print(f"S={S}: fixture slots: {excused} frames differ at recorded near ties (<= {n_near}); latent tail {e_lat:.2e}, wav head "
          f"{e_head:.2e}, wav tail {e_tail:.2e} (bound 1e-3); clipped slot vs oracle: {o_excused} frames at near ties, wav {e_clip:.2e} "
          f"(bound 1e-3)")
    assert excused <= n_near
    assert e_lat < 1e-3 and e_head < 1e-3 and e_tail < 1e-3
    assert e_clip < 1e-3
    assert torch.isfinite(wav).all()


@pytest.mark.parametrize("S", [32, 64])
def test_streams_are_independent(S):
    """The S-stream session again with every non-fixture slot's audio and codes replaced: the fixture slots' codes and waveforms are
    bit-identical (split-K plans, tile shapes and the RVQ chain's atomicMin order depend on sizes, not values; attention is per
    (stream, head); every history roll is per row)."""
    _, _, codes_a, wav_a = _cached_session(S, 0, eager=False)
    _, _, codes_b, wav_b = _cached_session(S, 1, eager=False)
    fx = [0, S - 1]
    others = [i for i in range(1, S - 1)]
    assert not torch.equal(codes_a[others], codes_b[others])       # the other slots did change
    dc = int((codes_a[fx] != codes_b[fx]).sum())
    dw = float((wav_a[fx] - wav_b[fx]).abs().max())
    print(f"S={S}: fixture slots across the two sessions: {dc} code entries differ, max |wav difference| {dw:.3e} (bound: 0, bit-identical)")
    assert dc == 0 and torch.equal(wav_a[fx], wav_b[fx])


# ------------------------------------------------------------------------------------------------------------ 3: kernels vs fp64

@functools.lru_cache(maxsize=8)
def _frame(S: int):
    sd, model = _mimi()
    return CS.record_frame(model, S, _card(sd))


def _unique(recs):
    seen, out = set(), []
    for r in recs:
        k = tuple(sorted(r.items()))
        if k not in seen:
            seen.add(k)
            out.append(r)
    return out


def _replay_gemm_win(r, g):
    """ops.gemm_win at the recorded sizes with random operands and a random, non-zero history per stream -> (measured backward error
    / 2^-24, route)."""
    B, T_in, T_out, C, S, P, N, K = (r[k] for k in ("B", "T_in", "T_out", "C", "S", "P", "N", "K"))
    assert r["hist"] == (P > 0), f"a streamed call with P = {P} and no history: {r}"
    x = torch.randn(B, T_in, C, generator=g)
    hist = (torch.randn(B, P, C, generator=g) + 0.5) * (1 + torch.arange(B)).view(B, 1, 1) if P else None
    res = torch.randn(B, T_out, N, generator=g) if r["res"] else None
    scale = torch.rand(N, generator=g) if r["scale"] else None
    seq = torch.cat([hist, x], 1).double() if P else x.double()
    a = F.elu(seq) if r["act_in"] == ops.ACT_ELU else seq
    if r["convtr"]:
        kernel, stride = r["convtr"]
        q, cout = -(-kernel // stride), N // stride
        assert P == q - 1 and K == q * C and res is None and scale is None
        wt = torch.randn(C, cout, kernel, generator=g) / math.sqrt(C * q)
        w = RF.pack_convtr_weight(wt, stride)
        b0 = 0.1 * torch.randn(cout, generator=g) if r["bias"] else None
        bias = b0.repeat(stride).contiguous() if b0 is not None else None
        crop = lambda y: y[:, :, (q - 1) * stride:(q - 1 + T_out) * stride].transpose(1, 2)   # [B, T_out * stride, cout]
        wt64 = F.pad(wt.double(), (0, q * stride - kernel))                      # zero taps up to q * stride: whole output blocks
        acc = crop(F.conv_transpose1d(a.transpose(1, 2), wt64, stride=stride))
        mag = crop(F.conv_transpose1d(a.abs().transpose(1, 2), wt64.abs(), stride=stride))
        ref, m = CS.epilogue64(acc, mag, b0.double() if b0 is not None else None, None, None, r["act_out"])
        shape = (B, T_out * stride, cout)
    else:
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        bias = 0.1 * torch.randn(N, generator=g) if r["bias"] else None
        A = CS.window_rows(a, K // C, S, T_out)
        acc, mag = A @ w.double().t(), A.abs() @ w.double().abs().t()
        ref, m = CS.epilogue64(acc, mag, bias.double() if bias is not None else None, res.double() if res is not None else None,
                               scale.double() if scale is not None else None, r["act_out"])
        shape = (B, T_out, N)
    d = lambda t: t.to(DEV) if t is not None else None
    ops.PROFILE = []
    try:
        y = ops.gemm_win(d(x), d(w), B=B, T_in=T_in, T_out=T_out, C_=C, S=S, P=P, N=N, hist=d(hist), bias=d(bias), res=d(res),
                         scale=d(scale), pad_mode=r["pad_mode"], act_in=r["act_in"], act_out=r["act_out"], out_shape=shape)
        torch.cuda.synchronize()
        names = [p[0] for p in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert names == [CS.key_of(r)[0]], (names, r)
    e = float(((y.double().cpu() - ref).abs() / (U * m).clamp_min(1e-300)).max())
    if P and names == ["gemm_skinny_f32"]:
        # the packing launch alone: the windows of [history ; chunk] (ELU on load), rows past M and columns past K zero
        M = B * T_out
        Kp = (K + 7) // 8 * 8
        xp = torch.full((32 if M <= 32 else (64 if M <= 64 else 128), Kp), float("nan"), device=DEV)
        xg, hg = d(x), d(hist)          # (held: a temporary's block could be handed to the next allocation before the launch)
        _lib.check(_lib.lib().rst_skinny_f32_pack_win(xg.data_ptr(), hg.data_ptr(), xp.data_ptr(), B, T_in, T_out, C, K, S, P,
                                                     r["pad_mode"], T_in * C, r["act_in"], torch.cuda.current_stream().cuda_stream))
        rows = CS.unpack_f32(xp, K).double().cpu()
        win = CS.window_rows(a, K // C, S, T_out).reshape(M, K)
        # ELU on load: e^x - 1 within 7e-8 absolute of the exact value (rst_common.h rst_elu), the identity elsewhere
        assert bool(((rows[:M, :K] - win).abs() <= 2 * U * win.abs() + 1e-7).all()), f"pack_win rows differ from the windows: {r}"
        assert not rows[M:].any() and not rows[:, K:].any(), f"pack_win: rows past M / columns past K are not zero: {r}"
    return e


def _replay_linear(r, g):
    """ops.linear at the recorded sizes / switches (LayerNorm folded into the packing, packed operand in, packed result out)."""
    M, N, K = r["M"], r["N"], r["K"]
    x = torch.randn(M, K, generator=g) + 0.3
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = 0.1 * torch.randn(N, generator=g) if r["bias"] else None
    res = torch.randn(M, N, generator=g) if r["res"] else None
    scale = 0.25 * torch.rand(N, generator=g) if r["scale"] else None           # LayerScale
    d = lambda t: t.to(DEV) if t is not None else None
    ln = None
    if r["ln"]:
        gam, bet = 1 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
        a, amag = CS.layernorm64(x, gam, bet, 1e-5)
        # the mean's own rounding moves every x - mean by up to ~K 2^-24 mean|x|: a term relative to rstd |gamma| mean|x|
        rstd = 1 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
        amag = amag + rstd * gam.double().abs() * x.double().abs().mean(-1, keepdim=True)
        ln = (d(gam), d(bet), 1e-5)
    if r["ln"] and "pack_ln" in CS.route_of(r):
        # the packing launch alone against the fp64 LayerNorm; rows past M zero
        Kp = (K + 7) // 8 * 8
        xp = torch.full((32 if M <= 32 else (64 if M <= 64 else 128), Kp), float("nan"), device=DEV)
        xg = d(x)
        _lib.check(_lib.lib().rst_skinny_f32_pack_ln(xg.data_ptr(), ln[0].data_ptr(), ln[1].data_ptr(), 1e-5, xp.data_ptr(), M, K,
                                                    torch.cuda.current_stream().cuda_stream))
        rows = CS.unpack_f32(xp, K).double().cpu()
        e_ln = float(((rows[:M, :K] - a).abs() / (U * amag)).max())
        print(f"    pack_ln M={M} K={K}: |LN - fp64| / (2^-24 (|x_hat gamma| + |beta| + rstd |gamma| mean|x|)) = {e_ln:.2f} (bound {C_GEMM:.0f})")
        assert e_ln <= C_GEMM and not rows[M:].any() and not rows[:, K:].any()
    if not r["ln"]:
        a, amag = x.double(), x.double().abs()
    xin = d(x)
    if r["packed_in"]:
        xp = CS.pack_rows(xin)
        assert not CS.unpack_f32(xp, K)[M:].any(), "packed operand: rows past M are not zero"
        xin = ops.PackedRows(xp, (M, K))
    ops.PROFILE = []
    try:
        y = ops.linear(xin, d(w), d(bias), res=d(res), scale=d(scale), act_out=r["act_out"], ln=ln, out_packed=r["out_packed"])
        torch.cuda.synchronize()
        names = [p[0] for p in ops.PROFILE]
    finally:
        ops.PROFILE = None
    if r["out_packed"]:
        y = CS.unpack_f32(y.xp, N)[:M, :N]
    acc, mag = a @ w.double().t(), amag @ w.double().abs().t()
    ref, m = CS.epilogue64(acc, mag, bias.double() if bias is not None else None, res.double() if res is not None else None,
                           scale.double() if scale is not None else None, r["act_out"])
    assert len(names) <= 1
    return float(((y.reshape(M, N).double().cpu() - ref).abs() / (U * m).clamp_min(1e-300)).max())


@pytest.mark.parametrize("S", [3, 9, 32, 64, 65])
def test_frame_gemms_at_real_shapes_vs_fp64(S):
    """Every ops.gemm_win / ops.linear call of one eager streamed frame (encode + decode) at S streams, replayed at its sizes,
    window form, padding, ELU on load and epilogue with random operands -- a random, non-zero history different per stream --
    against fp64: per-element backward error |y - ref| <= 16 * 2^-24 * (sum_k |x_k| |w_k| + |bias| + the epilogue's terms).
    Convolution windows against fp64 conv1d of [history ; chunk], transposed-convolution windows against fp64 conv_transpose1d."""
    enc, dec, _ = _frame(S)
    g = torch.Generator().manual_seed(S)
    rows, worst = [], 0.0
    for r in _unique(enc + dec):
        if r["kind"] not in ("gemm_win", "linear"):
            continue
        e = _replay_gemm_win(r, g) if r["kind"] == "gemm_win" else _replay_linear(r, g)
        M = r["B"] * r["T_out"] if r["kind"] == "gemm_win" else r["M"]
        form = ("convtr" if r.get("convtr") else "conv" if r["kind"] == "gemm_win" and r["K"] != r["C"] else "linear")
        extra = "".join(f" {k}" for k in ("hist", "ln", "packed_in", "out_packed", "res") if r.get(k)) + (" elu-in" if r.get("act_in") else "")
        rows.append((e, f"M={M} N={r['N']} K={r['K']} {form}{extra}: {CS.route_of(r)}"))
        worst = max(worst, e)
    for e, what in rows:
        print(f"  S={S} {what}: backward error / 2^-24 = {e:.2f} (bound {C_GEMM:.0f})")
    print(f"S={S}: {len(rows)} distinct calls, worst {worst:.2f} (bound {C_GEMM:.0f})")
    bad = [what for e, what in rows if not e <= C_GEMM]
    assert not bad, bad


# ---- the one-launch attention step

H_ATT, D_ATT, T_ATT = 8, 64, 2


def _rope64(x, ang):
    """Interleaved pairs of ``x [..., D]`` rotated in fp64 by the fp32 angles ``ang [D / 2]`` (broadcast over leading dims)."""
    xr, xi = x.double()[..., 0::2], x.double()[..., 1::2]
    c, s = torch.cos(ang.double()), torch.sin(ang.double())
    out = torch.empty(x.shape, dtype=torch.float64)
    out[..., 0::2], out[..., 1::2] = xr * c - xi * s, xr * s + xi * c
    return out


def _pair_norm(x):
    return torch.sqrt(x[..., 0::2] ** 2 + x[..., 1::2] ** 2)


def _attention_run(S, cap, context, pos0, steps, packed, g):
    """`steps` consecutive attention steps of T = 2 new positions from position pos0, rings pre-filled with the `cap` positions before
    pos0 (NaN where the ring holds nothing yet).  Returns (worst output error / bound, worst new-key error / bound)."""
    H, D, T = H_ATT, D_ATT, T_ATT
    coef = ops.rope_coef(10000.0, D)
    freq = torch.exp(torch.arange(D // 2, dtype=torch.float32) * torch.tensor(coef, dtype=torch.float32))   # modules/rope.py, fp32
    k = torch.full((S, H, cap, D), float("nan"))
    v = torch.full((S, H, cap, D), float("nan"))
    keys, eps_k = {}, {}        # position -> (key as stored [S, H, D] fp64, value fp64); position -> rotation error bound [S, H, D/2]
    for pk in range(max(0, pos0 - cap), pos0):
        kk, vv = torch.randn(S, H, D, generator=g), torch.randn(S, H, D, generator=g)
        k[:, :, pk % cap], v[:, :, pk % cap] = kk, vv
        keys[pk] = (kk.double(), vv.double())
        eps_k[pk] = torch.zeros(S, H, D // 2, dtype=torch.float64)
    kd, vd = k.to(DEV), v.to(DEV)
    pos_dev = torch.tensor([pos0], dtype=torch.int64, device=DEV)
    scale = 1.0 / math.sqrt(D)
    NC = 256 // (D // 4)
    n_acc = -(-cap // NC) + NC + 16          # o: per-thread chain over the slots of a class, then the classes; L: 256 threads to 1; the division
    worst_o = worst_k = 0.0
    for st in range(steps):
        p0 = pos0 + st * T
        qkv = torch.randn(S, T, 3 * H * D, generator=g)
        k_before, v_before = kd.cpu(), vd.cpu()
        out = ops.attention_step(qkv.to(DEV), H, kd, vd, pos_dev, context=context, rope=True, max_period=10000.0, out_packed=packed)
        pos_dev.add_(T)
        torch.cuda.synchronize()
        M = S * T
        if packed:
            rows = CS.unpack_f32(out.xp, H * D)
            assert not rows[M:].any(), "packed attention result: rows past M are not zero"
            got = rows[:M].reshape(S, T, H, D).cpu().double()
        else:
            got = out.reshape(S, T, H, D).cpu().double()
        q, kn, vn = qkv.view(S, T, 3, H, D).unbind(2)                                  # [S, T, H, D]
        ts = torch.tensor([float(p0)], dtype=torch.float32) + torch.arange(T, dtype=torch.float32)
        ang = freq[None, :] * ts[:, None]                                             # [T, D/2] fp32, as the reference computes it
        # one ulp of the frequency (GPU expf vs the reference's exp) and of the product move the angle by <= 2^-22 |angle|; the
        # rotation's two products, its sum and cos / sin add <= 8 ulp of the pair norm
        eps_rot = 2.0 ** -22 * ang.double().abs() + 8 * U                            # [T, D/2]
        k_after, v_after = kd.cpu(), vd.cpu()
        new_slots = [(p0 + t) % cap for t in range(T)]
        for t in range(T):
            kr = _rope64(kn[:, t], ang[t])
            keys[p0 + t] = (kr, vn[:, t].double())
            eps_k[p0 + t] = eps_rot[t].expand(S, H, D // 2)
            sl = new_slots[t]
            assert torch.equal(v_after[:, :, sl], vn[:, t]), f"ring v of position {p0 + t} is not the step's v"
            kb = (_pair_norm(kr) * eps_rot[t]).repeat_interleave(2, -1)
            ek = float(((k_after[:, :, sl].double() - kr).abs() / kb).max())
            worst_k = max(worst_k, ek)
        old = [s for s in range(cap) if s not in new_slots]
        assert torch.equal(k_after[:, :, old].nan_to_num(7.0), k_before[:, :, old].nan_to_num(7.0)), "the step wrote ring k slots it does not own"
        assert torch.equal(v_after[:, :, old].nan_to_num(7.0), v_before[:, :, old].nan_to_num(7.0)), "the step wrote ring v slots it does not own"
        end = p0 + T
        lo = max(0, end - cap + 1)          # once wrapped, the slot at end_index is labelled position end_offset: its key is not seen
        window = list(range(lo, end))
        Kw = torch.stack([keys[pk][0] for pk in window], 2)                            # [S, H, n, D]
        Vw = torch.stack([keys[pk][1] for pk in window], 2)
        Ew = torch.stack([eps_k[pk] for pk in window], 2)                              # [S, H, n, D/2]
        for t in range(T):
            p = p0 + t
            vis = torch.tensor([pk <= p and (context is None or p - pk < context) for pk in window])
            qr = _rope64(q[:, t], ang[t])                                              # [S, H, D]
            s = torch.einsum("shd,shnd->shn", qr, Kw) * scale
            s = s.masked_fill(~vis, float("-inf"))
            pr = torch.softmax(s, -1)
            o = torch.einsum("shn,shnd->shd", pr, Vw)
            # score error: rotation of q and of the new keys (pair norms x angle error), the D-term dot product, the max subtraction
            # and expf; to first order d o = sum_j p_j d s_j (v_j - o), so |d o| <= sum_j p_j e_j |v_j - o|; the sums of p v and p
            # (n_acc roundings) add n_acc 2^-24 sum_j p_j |v_j|
            qn = _pair_norm(qr)
            e = scale * torch.einsum("shp,shnp->shn", qn * eps_rot[t], _pair_norm(Kw)) \
                + scale * torch.einsum("shp,shnp->shn", qn, _pair_norm(Kw) * Ew) \
                + scale * D * U * torch.einsum("shd,shnd->shn", qr.abs(), Kw.abs()) \
                + U * (4 + (s - s.max(-1, keepdim=True).values).abs().nan_to_num(0.0, 0.0, 0.0))
            bound = 1.01 * torch.einsum("shn,shnd->shd", pr * e, (Vw - o[:, :, None]).abs()) \
                + n_acc * U * torch.einsum("shn,shnd->shd", pr, Vw.abs())
            eo = float(((got[:, t] - o).abs() / bound).max())
            worst_o = max(worst_o, eo)
    return worst_o, worst_k


@pytest.mark.parametrize("cap,context", [(250, 250), (250, 100)], ids=["ring250_ctx250", "ring250_ctx100"])
@pytest.mark.parametrize("S", [3, 9, 32, 64, 65])
def test_attention_step_vs_fp64_ring_attention(S, cap, context):
    """rst_attention_step_f32 at S streams, 8 heads of 64, 2 new positions per step (Mimi's transformers at 12.5 Hz x 2), row-major
    and packed result (M = 2S <= 128), three consecutive steps from: an empty ring (its unused slots NaN: never read), a step whose
    two positions straddle the wrap (pos0 = cap - 1), deep steady state (pos0 = 40 cap).  Reference: the reference's ring semantics
    (oracle/mimi_oracle.py RingKVCache.complete + ring_attention: the ring holds the last cap positions, and once it has wrapped the
    slot at end_index is labelled position end_offset, so that key is not seen) with the RoPE angle in fp32 as modules/rope.py
    computes it and everything after it in fp64.  Bounds per element, derived in _attention_run; ring v bit-exact, ring k within
    the rotation bound, every other slot untouched."""
    forms = [False, True] if S * T_ATT <= ops.SKINNY_F32_MAX_ROWS else [False]
    g = torch.Generator().manual_seed(1000 + S + cap + context)
    for pos0 in (0, cap - 1, 40 * cap):
        for packed in forms:
            eo, ek = _attention_run(S, cap, context, pos0, 3, packed, g)
            print(f"S={S} cap={cap} context={context} pos0={pos0} {'packed' if packed else 'row-major'}: output error / bound {eo:.3f}, "
                  f"new ring keys error / bound {ek:.3f} (both <= 1)")
            assert eo <= 1.0 and ek <= 1.0, (pos0, packed, eo, ek)


# ------------------------------------------------------------------------------------------------------------ 4: coverage

GEMM_NAMES = ("gemm_win", "gemm_win_b3", "gemm_skinny_f32")


@pytest.mark.parametrize("S", [3, 9, 32, 64, 65])
def test_frame_routes_are_the_ones_covered(S):
    """ops.PROFILE of one eager streamed frame: every GEMM launch (name, M, N, K) is one of the calls test_frame_gemms_at_real_shapes_vs_fp64
    replays; the routes that test relies on hold (the layer loop, not codec_tr, for S > 2; the one-launch attention step at the shape
    test_attention_step_vs_fp64_ring_attention covers; f32 gemm_win, never the three-plane form, for every call with a history;
    the route crossings of the module docstring)."""
    _, model = _mimi()
    enc, dec, prof = _frame(S)
    recs = enc + dec
    covered = {CS.key_of(r) for r in recs} - {None}
    missing = [p for p in prof if p[0] in GEMM_NAMES and (p[0],) + p[1] not in covered]
    assert not missing, f"S={S}: GEMM launches no replayed call covers: {missing}"
    # the three-plane kernel takes the history-free launches of more than 4096 rows (from S = 43 on, the 1x1 convolution of 96 rows per
    # stream); never one with a history (rst_gemm_win_b3_supported)
    b3 = {p for p in prof if p[0] == "gemm_win_b3"}
    assert all(not r["hist"] for r in recs if CS.key_of(r) is not None and (CS.key_of(r)[0], CS.key_of(r)[1:]) in b3), b3
    other = sorted({p[0] for p in prof} - set(GEMM_NAMES))
    assert other in ([], ["resblock"]), other      # the fused SEANet residual blocks (streaming form, with history), tested in test_mimi_gpu
    prof_set = set(prof)
    for r in recs:
        if r["kind"] == "gemm_win" and r["hist"]:
            key = CS.key_of(r)
            assert (key[0], key[1:]) in prof_set and ("gemm_win_b3", key[1:]) not in prof_set, f"S={S}: a call with a history: {r}"
    tr = model.encoder_transformer.transformer
    l0 = tr.layers[0]
    E, Hh = l0.self_attn.out_proj.weight.shape[0], l0.self_attn.num_heads
    att = [r for r in recs if r["kind"] == "attention_step"]
    assert len(att) == 2 * len(tr.layers), f"S={S}: {len(att)} attention steps in a frame (one per layer of both transformers expected)"
    assert {(r["B"], r["T"], r["H"], r["D"], r["cap"], r["context"]) for r in att} == {(S, T_ATT, H_ATT, D_ATT, 250, 250)}
    assert ops.attention_step_supported(torch.empty(S, T_ATT, 3 * E, device=DEV), Hh, 250)
    assert not ops.codec_transformer_frame_supported(S, T_ATT, E, Hh, l0.linear1.out_features, len(tr.layers), 250)
    routes = sorted({CS.route_of(r) for r in recs})
    print(f"S={S} routes:\n  " + "\n  ".join(routes))
    # the crossings of the module docstring, from the library's own plans
    gw = [r for r in recs if r["kind"] == "gemm_win"]
    if S == 9:
        assert any(r["hist"] and "under-filled" in CS.route_of(r) for r in gw), "S=9: no under-filled 128 x 128 launch with a history"
    if S == 64:
        assert any(r["kind"] == "linear" and r["M"] == 128 and CS.route_of(r).startswith("skinny") for r in recs)
    if S == 65:
        lin = [r for r in recs if r["kind"] == "linear" and r["M"] == 130]
        assert lin and not any(CS.route_of(r).startswith("skinny") for r in lin)
    if S <= 64:
        assert all(not (r["kind"] == "linear" and r["M"] == 2 * S) or CS.route_of(r).startswith("skinny") for r in recs)
