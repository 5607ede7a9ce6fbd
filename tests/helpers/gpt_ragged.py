"""Shared pieces of tests/test_gpt_ragged_cpu.py and tests/test_gpt_ragged_gpu.py: the six TTS prompts of the batched-generation test,
their per-stream noise, and the CPU oracle's generation of each prompt WITH its decision margins.  Nothing here needs a GPU.

Margins (what an identity test against the oracle rests on):
  greedy   (top1 - top2) / max|logit| of every argmax the oracle takes;
  sampled  (r1 - r2) / r1 of the two largest race terms r_j = p_j / noise_j over the sorted top-k.
tests/test_gpt_gpu.py quotes about 1e-6 of summation-order noise between the product and the oracle on these models; the CPU test holds
every margin at >= MARGIN = 1e-4, one hundred times that."""
import functools

import torch

from oracle import gpt_generate_oracle as GG
from oracle import gpt_oracle as Gp
from rstnet_amd import synth
from tests.golden import cases

CFGS = {"gqa": synth.GPT_TINY_GQA, "mha": synth.GPT_TINY_MHA}
# (L, n_text, n_pad, seed) of each prompt, in the layout of tests/test_gpt_gpu.py::_tts_prompt
PROMPTS = [(10, 1, 2, 0), (14, 4, 2, 1), (16, 5, 2, 2), (20, 11, 3, 3), (24, 12, 2, 4), (30, 17, 4, 5)]
IDS = dict(text_pad_token=319, text_empty_token=318, semantic_pad_token=31, n_audio_codes=30)
TEXT_INIT = 151655 % 320
SAMPLING = dict(temp=0.8, top_k=8, temp_text=0.7, top_k_text=5)
MARGIN = 1e-4


def tts_prompt(cfg_d, L, n_text, n_pad, seed):
    """A [K, L] utterance in the reference's TTS layout: text ids then `text_empty` on row 0, audio rows, trailing padding."""
    g = torch.Generator().manual_seed(seed)
    K = cfg_d["n_q"] + 1
    seq = torch.randint(0, 30, (K, L), generator=g)
    seq[0, :n_text] = torch.randint(0, 300, (n_text,), generator=g)
    seq[0, n_text:] = 318
    seq[1:, L - n_pad:] = 31
    return seq


def prompts(cfg_d):
    return [tts_prompt(cfg_d, *p) for p in PROMPTS]


def stream_noise(b, k_text=SAMPLING["top_k_text"], k_audio=SAMPLING["top_k"]):
    """Exp(1) draws of stream ``b``: ``(kind, g_idx, l_idx) -> [1, k]``."""
    def fn(kind, g_idx, l_idx):
        g = torch.Generator().manual_seed(100000 * b + 1000 * g_idx + 10 * l_idx + (kind == "text"))
        return -torch.log(torch.rand(1, k_text if kind == "text" else k_audio, generator=g).clamp_min(1e-9))
    return fn


def batch_noise(B):
    """The hook of a batched generation: row ``b`` is stream ``b``'s draw -> ``[B, k]``."""
    fns = [stream_noise(b) for b in range(B)]
    return lambda kind, g_idx, l_idx: torch.cat([f(kind, g_idx, l_idx) for f in fns], 0)


def oracle_config(cfg_d):
    keep = set(Gp.GPTConfig.__dataclass_fields__)
    return Gp.GPTConfig(**{k: v for k, v in cfg_d.items() if k in keep})


@functools.lru_cache(maxsize=None)
def cpu_merged_state(name):
    """The merged fp32 state dict the oracle is fed, from the product's own loader on the CPU (no kernel runs there)."""
    from rstnet_amd.lm.gpt import GPT, Config
    cfg_d = dict(CFGS[name])
    model = GPT.from_state_dict(synth.gpt_state_dict(cfg_d, cases.GPT_SEED), Config.from_dict(cfg_d))
    return {k: v.detach().float() for k, v in model.state_dict().items()}


def oracle_generate(osd, ocfg, cfg_d, sampled):
    """``GG.generate`` of each of the six prompts alone (stream ``b`` on its own noise) -> (list of result dicts, smallest margin of any
    decision).  The margin is read by wrapping the oracle's ``sample_token``; its decisions are untouched."""
    real = GG.sample_token
    worst = [float("inf")]

    def recording(logits, use_sampling, temp, top_k, noise, limit=0):
        if use_sampling and temp > 0.0:
            probs = torch.softmax(logits / temp, dim=-1)
            if limit:
                probs[..., limit:] = float("-inf")
            p, _ = torch.topk(probs, top_k, dim=-1)
            r, _ = torch.topk((p / noise).reshape(-1), 2)
            worst[0] = min(worst[0], float((r[0] - r[1]) / r[0]))
        else:
            t, _ = torch.topk(logits.reshape(-1), 2)
            worst[0] = min(worst[0], float((t[0] - t[1]) / logits.abs().max()))
        return real(logits, use_sampling, temp, top_k, noise, limit)

    outs = []
    GG.sample_token = recording
    try:
        for b, seq in enumerate(prompts(cfg_d)):
            nz = stream_noise(b)
            outs.append(GG.generate(osd, ocfg, seq, "TTS", use_sampling=sampled, ids=GG.GenIds(text_initial_token_id=TEXT_INIT, **IDS),
                                    noise=lambda kind, g, l: nz(kind, g, l).view(1, 1, -1) if kind == "text" else nz(kind, g, l).view(1, 1, 1, -1),
                                    **SAMPLING))
    finally:
        GG.sample_token = real
    return outs, worst[0]


@functools.lru_cache(maxsize=None)
def cpu_oracle_runs(name, sampled):
    """The oracle on the CPU-built merged weights: computed once per (config, mode), shared, never modified."""
    cfg_d = dict(CFGS[name])
    return oracle_generate(cpu_merged_state(name), oracle_config(cfg_d), cfg_d, sampled)
