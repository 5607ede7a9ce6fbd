"""Shared pieces of tests/test_slot_server_cpu.py and tests/test_slot_server_gpu.py: the slot-server scenario (three rows, 14 ticks, the
tiny 16-stream LM behind the synthetic Mimi), what every client sends, and the CPU oracles' run of every conversation WITH the margins of
its greedy decisions.  Nothing here needs a GPU.

  tick      0  1  2  3  4  5  6  7  8  9 10 11 12 13
  row 0     A  A  A  A  A  A  A  .  C  C  C  C  C  C        A (f32) joins before tick 0 and leaves after tick 6; C (f32) joins before tick 8
  row 1     .  .  B  B  -  B  B  B  B  B  B  B  B  B        B (s16) joins before tick 2 and misses its frame at tick 4 (fed silence)
  row 2     .  .  .  .  .  .  .  .  .  .  .  .  .  .        never taken

The GPU test compares tokens between two GPU runs whose neighbours differ; that rests on the decisions not being ties, which the CPU test
holds to MARGIN = 1e-4 (tests/helpers/stream_restart.py) on the oracles' logits for exactly these inputs."""
import functools

import numpy as np
import torch

from rstnet_amd import synth

FRAME = 1920
N, TICKS = 3, 14
LM_SEED, MIMI_SEED = 9, 0
MARGIN = 1e-4
# (audio seeds chosen so that the margins hold: 1.9e-3, 1.9e-3 and 1.4e-3 for A, B and C; seeds 42 and 44 put B at 4e-5 and 7e-5)
# name -> (row, format, tick of the first frame, tick after the last one, ticks without a frame, audio seed)
CLIENTS = {
    "A": (0, "f32", 0, 7, (), 41),
    "B": (1, "s16", 2, TICKS, (4,), 45),
    "C": (0, "f32", 8, TICKS, (), 43),
}


def cfg():
    return dict(synth.LM_TINY_16Q)


@functools.lru_cache(maxsize=None)
def payloads(name: str):
    """What client ``name`` sends: per tick of its conversation the payload bytes of one frame in its transport, ``None`` where it misses."""
    _, fmt, t0, t1, missed, seed = CLIENTS[name]
    pcm = synth.synth_audio(1, (t1 - t0) * FRAME, seed=seed)[0, 0].numpy()
    out = []
    for i in range(t1 - t0):
        fr = pcm[i * FRAME:(i + 1) * FRAME]
        if t0 + i in missed:
            out.append(None)
        elif fmt == "f32":
            out.append(fr.astype("<f4").tobytes())
        else:
            out.append((np.clip(fr, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())
    return out


def heard(name: str) -> torch.Tensor:
    """fp32 ``[1, 1, frames * FRAME]``: the conversation as the model hears it -- s16 through ``x / 32768``, silence where a frame is missed."""
    fmt = CLIENTS[name][1]
    rows = []
    for p in payloads(name):
        if p is None:
            rows.append(np.zeros(FRAME, dtype=np.float32))
        elif fmt == "f32":
            rows.append(np.frombuffer(p, dtype="<f4").copy())
        else:
            rows.append(np.frombuffer(p, dtype="<i2").astype(np.float32) / 32768.0)
    return torch.from_numpy(np.concatenate(rows))[None, None]


@functools.lru_cache(maxsize=1)
def oracle_margin() -> float:
    """Smallest margin (top1 - top2) / max|logit| of any greedy decision the composed oracles take on the three conversations."""
    from oracle import lm_oracle as L
    from oracle import mimi_oracle as O
    mimi_sd = synth.mimi_state_dict(MIMI_SEED)
    sd = {k: v.float() for k, v in synth.lm_state_dict(cfg(), seed=LM_SEED).items()}
    real = L.sample_token
    worst = [float("inf")]

    def recording(logits, use_sampling, temp, top_k, noise=None, top_p=0.0):
        t, _ = torch.topk(logits.reshape(logits.shape[0], -1) if logits.dim() > 1 else logits.reshape(1, -1), 2)
        worst[0] = min(worst[0], float(((t[:, 0] - t[:, 1]) / logits.abs().max()).min()))
        return real(logits, use_sampling, temp, top_k, noise, top_p)

    L.sample_token = recording
    try:
        with torch.no_grad():
            for name in CLIENTS:
                x = heard(name)
                codes = O.encode(mimi_sd, O.MimiConfig(), x)
                ora = L.LMGenOracle(sd, L.LMConfig(**cfg()), 1)
                for f in range(codes.shape[-1]):
                    ora.step(codes[:, :, f:f + 1])
    finally:
        L.sample_token = real
    return worst[0]
