"""Shared pieces of tests/test_stream_sampling_cpu.py and tests/test_stream_sampling_gpu.py: the noise of
``rst_noise_exp_ps_f32`` in numpy (Philox4x32-10, the exact uniform, ``-log u`` in fp64), the decision margins of a sampler call, and the
three scenarios of the GPU tests -- sampler rows, an ``LMGen`` session of three streams, the slot server -- with the CPU oracle's run of
every conversation in them.  Nothing here needs a GPU.

Margins.  The GPU tests compare TOKENS: between GPU runs whose neighbours differ, and with the oracle fed numpy noise.  That rests on no
decision being a near-tie, which the CPU test holds to MARGIN = 1e-4 (the bar of tests/helpers/stream_restart.py) at every sampler call:
  greedy      (top1 - top2) / max|logit|
  sampling    (r1 - r2) / r1 over the race terms r_j = p_j / noise_j of the k candidates, and (p_k - p_{k+1}) / p_k, the edge of the top-k
against a device noise within 4 ulp (2.4e-7 relative) of the numpy one and summation-order differences of ~1e-6."""
import functools

import numpy as np
import torch

from oracle import lm_oracle as L
from rstnet_amd import synth
from tests.helpers import slot_server as SS

MARGIN = 1e-4
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
KAT_ZERO = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)      # Philox4x32-10 of an all-zero counter and key (Random123 kat_vectors)
MASK = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------- the noise, in numpy

def philox4x32_10(counter: np.ndarray, key: np.ndarray) -> np.ndarray:
    """``counter`` uint32 ``[..., 4]``, ``key`` uint32 ``[..., 2]`` (broadcast against each other) -> uint32 ``[..., 4]``."""
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.asarray(key[..., 0], dtype=np.uint64), np.asarray(key[..., 1], dtype=np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & MASK, (k1 + np.uint64(PHILOX_W1)) & MASK
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def uniform_of(x: np.ndarray) -> np.ndarray:
    """The launch's uniform of a Philox word, exactly, in fp64: ``((x >> 9) + 0.5) * 2^-23`` -- a 24-bit number, so fp32 holds it too."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def words(seed: int, frame: int, n_cols: int) -> np.ndarray:
    """The Philox words of columns ``0 .. n_cols - 1`` of a row with this seed (0 .. 2^64 - 1) and frame counter."""
    seed, frame = int(seed) & (2 ** 64 - 1), int(frame) & (2 ** 64 - 1)
    q = np.arange((n_cols + 3) // 4, dtype=np.uint32)
    ctr = np.stack([q, np.zeros_like(q), np.full_like(q, frame & 0xFFFFFFFF), np.full_like(q, frame >> 32)], -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    return philox4x32_10(ctr, key[None, :]).reshape(-1)[:n_cols]


def noise_f64(seed: int, frame: int, n_cols: int) -> np.ndarray:
    """``-log(u)`` in fp64 of the exact ``u``: what ``noise[b][0 .. n_cols)`` approximates."""
    return -np.log(uniform_of(words(seed, frame, n_cols)))


def noise_f32(seed: int, frame: int, n_cols: int) -> torch.Tensor:
    """The same rounded to fp32: the noise the oracle is fed."""
    return torch.from_numpy(noise_f64(seed, frame, n_cols).astype(np.float32))


def ulp_distance(got_f32: np.ndarray, want_f64: np.ndarray) -> np.ndarray:
    """|got - want| in units of the fp32 spacing at ``want``."""
    want32 = want_f64.astype(np.float32)
    return np.abs(got_f32.astype(np.float64) - want_f64) / np.spacing(np.abs(want32)).astype(np.float64)


# -------------------------------------------------------------------------------------------------------------------------- margins

def call_margins(logits: torch.Tensor, use_sampling: bool, temp: float, top_k: int, noise) -> float:
    """The smallest margin of one ``sample_token`` call on one row of logits (see the module text)."""
    lg = logits.reshape(-1).float()
    if not (use_sampling and temp > 0.0):
        t, _ = torch.topk(lg, 2)
        return float((t[0] - t[1]) / lg.abs().max())
    probs = torch.softmax(lg / temp, dim=-1)
    k = min(int(top_k), lg.numel())
    p, _ = torch.topk(probs, min(k + 1, lg.numel()))
    worst = float("inf")
    if k < lg.numel():
        worst = min(worst, float((p[k - 1] - p[k]) / p[k - 1]))
    if k > 1:
        r, _ = torch.topk(p[:k] / torch.as_tensor(noise).reshape(-1)[:k], 2)
        worst = min(worst, float((r[0] - r[1]) / r[0]))
    return worst


class recording_margins:
    """``with recording_margins() as rec:`` -- every ``L.sample_token`` call inside reports to ``rec.worst`` / ``rec.calls``; decisions untouched."""

    def __enter__(self):
        self.real, self.worst, self.calls = L.sample_token, float("inf"), 0

        def recording(logits, use_sampling, temp, top_k, noise=None, top_p=0.0):
            self.worst = min(self.worst, call_margins(logits, use_sampling, temp, top_k, noise))
            self.calls += 1
            return self.real(logits, use_sampling, temp, top_k, noise, top_p)

        L.sample_token = recording
        return self

    def __exit__(self, *exc):
        L.sample_token = self.real
        return False


# ------------------------------------------------------------------------------------------------- scenario 1: rows of one sampler call

SAMPLER_V = (50, 2048, 4100)
SAMPLER_SEEDS = (11, 12, 2 ** 63 + 5, 14)       # noise seeds of the four rows
SAMPLER_FRAME = 3
# logits seed per V: the first one tried keeps the margins with and without the limits (observed minimum 1.2e-3, at V = 4100)
SAMPLER_LOGIT_SEED = {50: 0, 2048: 0, 4100: 0}


def sampler_cap(V: int) -> int:
    return 25 if V == 50 else 250


def sampler_rows(V: int):
    """``[(temperature, top_k)]`` of the four rows: greedy | top-1 | the cap | in between."""
    return [(0.0, 3), (0.5, 1), (1.0, sampler_cap(V)), (0.8, 7)]


def sampler_limits(V: int):
    """Per-row id limits of the second pass (each at least the cap, so that ``sample_token`` on the row cut at its limit is the reference)."""
    return [V, V - 7, sampler_cap(V) + 5, V // 2 + 1]


@functools.lru_cache(maxsize=None)
def sampler_logits(V: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 * V + SAMPLER_LOGIT_SEED[V])
    return torch.randn(4, V, generator=g) * 2.0


def sampler_reference(V: int, limits: bool):
    """-> (tokens the oracle draws for the four rows, the smallest margin).  With ``limits`` a row is cut at its limit: the blanking zeroes
    probabilities after the softmax, a common positive divisor of what is left, which changes neither the order nor the race."""
    logits, cap = sampler_logits(V), sampler_cap(V)
    toks, worst = [], float("inf")
    for b, (temp, k) in enumerate(sampler_rows(V)):
        row = logits[b, :sampler_limits(V)[b]] if limits and temp > 0.0 else logits[b]
        nz = noise_f32(SAMPLER_SEEDS[b], SAMPLER_FRAME, cap)[:k]
        worst = min(worst, call_margins(row, temp > 0.0, temp, k, nz))
        toks.append(int(L.sample_token(row[None], temp > 0.0, temp, k, nz[None])[0]))
    return toks, worst


# --------------------------------------------------------------------------------------------------- scenario 2: an LMGen session

CFG = dict(synth.LM_TINY)            # context 10: the temporal ring wraps at frame 10; delays [0, 0, 1, 0, 1]
B, FRAMES = 3, 14
TOP_K_CAP, TOP_K_TEXT_CAP = 8, 10    # the session's LMGen(top_k=, top_k_text=): the caps, and the noise layout [10 | 8 | 8]
RESET_ROW, RESET_FRAME = 1, 6
SWITCH_ROW, SWITCH_FRAME, SWITCH = 2, 9, dict(temp=1.1, top_k=7)
# (LM, user-token and row seeds chosen on the CPU so that every sampler call of every conversation below keeps the margins: smallest
# observed 1.9e-4 over the 168 calls; the first seeds tried)
LM_SEED, USER_SEED = 3, 0
ROWS = [
    dict(use_sampling=False, temp=0.8, temp_text=0.7, top_k=8, top_k_text=10, seed=101),
    dict(use_sampling=True, temp=1.0, temp_text=0.9, top_k=5, top_k_text=3, seed=2 ** 63 + 102),
    dict(use_sampling=True, temp=0.6, temp_text=0.7, top_k=4, top_k_text=6, seed=103),
]
# the second session of (b): other settings and seeds for whoever is not the row under test
OTHER = dict(use_sampling=True, temp=1.3, temp_text=0.4, top_k=2, top_k_text=9, seed=77)


def lm_state():
    return synth.lm_state_dict(CFG, LM_SEED)


def user_tokens(seed: int = USER_SEED) -> torch.Tensor:
    """int64 ``[FRAMES, B, Ki, 1]``: what the users say."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, CFG["card"], (FRAMES, B, CFG["n_q"] - CFG["dep_q"], 1), generator=g)


def frame_noise(seed: int, frame: int, dep_q: int, top_k_cap: int, top_k_text_cap: int, top_k: int, top_k_text: int, noise_fn=noise_f32):
    """The oracle's noise of one frame of a stream: ``(noise_text [top_k_text], [noise of depth step k: [top_k]])`` cut from the frame's
    columns -- text first, then ``dep_q`` blocks of ``top_k_cap`` -- a stream with a smaller top-k reads the head of each block.
    ``noise_fn(seed, frame, n_cols)`` -> fp32 ``[n_cols]``: the numpy noise, or (the GPU test) what the launch wrote."""
    nz = noise_fn(seed, frame, top_k_text_cap + dep_q * top_k_cap)
    return nz[:top_k_text], [nz[top_k_text_cap + k * top_k_cap:top_k_text_cap + k * top_k_cap + top_k] for k in range(dep_q)]


def oracle_conversation(sd, cfg: dict, user: torch.Tensor, settings: dict, caps, switch=None, noise_fn=noise_f32):
    """``LMGenOracle`` alone on one stream: ``user`` int64 ``[frames, 1, Ki, 1]``; ``settings`` as ``set_stream_sampling`` takes them;
    ``switch = (frame, changes)`` applies ``changes`` from that frame on.  -> per frame ``None`` or int64 ``[1, dep_q + 1, 1]``."""
    s = dict(settings)
    ora = L.LMGenOracle(sd, L.LMConfig(**cfg), 1, use_sampling=s["use_sampling"], temp=s["temp"], temp_text=s["temp_text"],
                        top_k=s["top_k"], top_k_text=s["top_k_text"])
    out = []
    for f in range(user.shape[0]):
        if switch is not None and f == switch[0]:
            s.update(switch[1])
            ora.use_sampling, ora.temp, ora.temp_text, ora.top_k, ora.top_k_text = s["use_sampling"], s["temp"], s["temp_text"], s["top_k"], s["top_k_text"]
        nt, na = frame_noise(s["seed"], f, cfg["dep_q"], caps[0], caps[1], s["top_k"], s["top_k_text"], noise_fn)
        out.append(ora.step(user[f], nt, na))
    return out


@functools.lru_cache(maxsize=1)
def lmgen_oracle_runs():
    """-> ({conversation: per-frame oracle output}, smallest margin, sampler calls).  Conversations: ``0``, ``1``, ``2`` (the rows of the
    undisturbed session) and ``"switch"`` (row 2 with SWITCH from SWITCH_FRAME on).  Computed once, shared, never modified."""
    sd = {k: v.float() for k, v in lm_state().items()}
    user = user_tokens()
    runs = {}
    with recording_margins() as rec, torch.no_grad():
        for b in range(B):
            runs[b] = oracle_conversation(sd, CFG, user[:, b:b + 1], ROWS[b], (TOP_K_CAP, TOP_K_TEXT_CAP))
        runs["switch"] = oracle_conversation(sd, CFG, user[:, SWITCH_ROW:SWITCH_ROW + 1], ROWS[SWITCH_ROW], (TOP_K_CAP, TOP_K_TEXT_CAP),
                                             switch=(SWITCH_FRAME, SWITCH))
    return runs, rec.worst, rec.calls


# ------------------------------------------------------------------------------------------------------ scenario 3: the slot server

# The scenario of tests/helpers/slot_server.py (rows, formats, ticks, joins, the missed frame, the leave) with sampling on and every
# client bringing its own settings.  The server keeps LMGen's defaults (top_k 250, top_k_text 25: the caps).
SLOT_LM_SEED, SLOT_MIMI_SEED = SS.LM_SEED, SS.MIMI_SEED
# (settings and seeds checked on the CPU for the margins: smallest observed 1.7e-4 over the 225 calls; the first ones tried)
SLOT_SAMPLING = {
    "A": dict(temp=0.9, temp_text=0.7, top_k=6, top_k_text=4, seed=5),
    "B": dict(temp=0.7, temp_text=0.8, top_k=12, top_k_text=3, seed=2 ** 64 - 2),
    "C": dict(use_sampling=False, seed=9),
}


def slot_settings(name: str) -> dict:
    """Client ``name``'s full settings: its own over the server's defaults."""
    return dict(dict(use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25), **SLOT_SAMPLING[name])


@functools.lru_cache(maxsize=1)
def slot_oracle_margin():
    """-> (smallest margin, sampler calls) of the composed oracles on the three conversations, each with its client's settings and noise."""
    from oracle import mimi_oracle as O
    cfg = SS.cfg()
    mimi_sd = synth.mimi_state_dict(SLOT_MIMI_SEED)
    sd = {k: v.float() for k, v in synth.lm_state_dict(cfg, seed=SLOT_LM_SEED).items()}
    n_user = cfg["n_q"] - cfg["dep_q"]
    with recording_margins() as rec, torch.no_grad():
        for name in SS.CLIENTS:
            codes = O.encode(mimi_sd, O.MimiConfig(), SS.heard(name))                  # [1, K, frames]
            user = codes[:, :n_user].permute(2, 0, 1)[..., None].contiguous()         # [frames, 1, Ki, 1]
            oracle_conversation(sd, cfg, user, slot_settings(name), (250, 25))
    return rec.worst, rec.calls
