"""Shared pieces of tests/test_stream_restart_cpu.py and tests/test_stream_restart_gpu.py: the LMGen restart scenario (LM_TINY, three
streams, 14 frames, stream 2 reset before frame 5), its user tokens, and the CPU oracle's run of every conversation in it WITH the
decision margins.  Nothing here needs a GPU.

A conversation is one stream between two (re)starts; the oracle runs each alone (streams are independent):
  stream 0, stream 1   frames 0 .. 13
  stream 2             frames 0 .. 4, then -- a new conversation -- frames 5 .. 13
Margin of a greedy decision: (top1 - top2) / max|logit| of every argmax the oracle takes (tests/helpers/gpt_ragged.py).  The GPU test
compares tokens with the oracle's, which rests on these margins; the CPU test holds them at >= MARGIN = 1e-4, about one hundred times
the summation-order noise between the product and the oracle on these models (tests/test_gpt_gpu.py quotes 1e-6)."""
import functools

import torch

from oracle import lm_oracle as L
from rstnet_amd import synth

CFG = dict(synth.LM_TINY)           # context 10 (the temporal ring wraps at frame 10), delays [0, 0, 1, 0, 1]: max delay 1
LM_SEED = 3
USER_SEED = 0
B, FRAMES, RESET_ROW, RESET_FRAME = 3, 14, 2, 5
MARGIN = 1e-4


def lm_state():
    return synth.lm_state_dict(CFG, LM_SEED)


def user_tokens() -> torch.Tensor:
    """int64 ``[FRAMES, B, Ki, 1]``: what the users say."""
    g = torch.Generator().manual_seed(USER_SEED)
    return torch.randint(0, CFG["card"], (FRAMES, B, CFG["n_q"] - CFG["dep_q"], 1), generator=g)


def conversations():
    """``[(stream, first frame, last frame + 1)]`` of the scenario."""
    return [(0, 0, FRAMES), (1, 0, FRAMES), (RESET_ROW, 0, RESET_FRAME), (RESET_ROW, RESET_FRAME, FRAMES)]


@functools.lru_cache(maxsize=1)
def oracle_runs():
    """-> ({(stream, first frame): [per frame: None or int64 [1, dep_q + 1, 1]]}, smallest margin of any decision).  Computed once, shared,
    never modified.  The margin is read by wrapping the oracle's ``sample_token``; its decisions are untouched."""
    sd = {k: v.float() for k, v in lm_state().items()}
    user = user_tokens()
    real = L.sample_token
    worst = [float("inf")]

    def recording(logits, use_sampling, temp, top_k, noise=None, top_p=0.0):
        t, _ = torch.topk(logits.reshape(-1), 2)
        worst[0] = min(worst[0], float((t[0] - t[1]) / logits.abs().max()))
        return real(logits, use_sampling, temp, top_k, noise, top_p)

    runs = {}
    L.sample_token = recording
    try:
        with torch.no_grad():
            for b, f0, f1 in conversations():
                ora = L.LMGenOracle(sd, L.LMConfig(**CFG), 1)
                runs[(b, f0)] = [ora.step(user[f, b:b + 1]) for f in range(f0, f1)]
    finally:
        L.sample_token = real
    return runs, worst[0]
