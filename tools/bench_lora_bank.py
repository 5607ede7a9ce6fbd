"""A/B of the batch-32 GPT frame (bench.py's ``gpt_b32`` shape) with the LoRA adapters merged, unmerged as ONE set, and served per
stream from a device-resident adapter bank (GPT.load_adapter_bank): one process, legs interleaved.

    python tools/bench_lora_bank.py [--repeats 7] [--samples 30] [--lm-config qwen0.5b|tiny] [--batch 32] [--out profiles/lora_bank_ab.json]

Legs, each a fresh ``GPTGen`` session (prompt of 8 positions, first frame, 10 warm-up frames, then ``--samples`` individually synchronised
graph-replayed ``GPTGen.step`` frames; the leg's figure is their median, bench.py's ``timing``):
  (a) merged      the default model: adapters merged into the dense weights at load
  (b) unmerged    the existing single-adapter ``merge_lora=False`` route (two thin matrix-core products behind every adapted linear)
  (c) bank_1of4   a bank of 4 sets, all rows on set 1
  (d) bank_32     a bank of B sets, row b on set b
  (e) bank_none   the bank of B sets, every row -1 (the base model: the launches run and return at once)
The round (a, b, c, d, e) is repeated ``--repeats`` times; reported per leg: the median over the rounds, and the ratios (c) / (b),
(d) / (a), (e) / (a).  Writes the JSON line to ``--out`` and prints it."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from rstnet_amd import _lib, synth  # noqa: E402
from rstnet_amd.lm.generate import GPTGen  # noqa: E402
from rstnet_amd.lm.gpt import GPT, Config  # noqa: E402

WARMUP = 10


def is_lora(k: str) -> bool:
    return k.endswith((".lora_A", ".lora_B"))


def random_sets(own: dict, n: int, dev) -> list:
    """``n`` adapter sets shaped and scaled like the state dict's own (uniform, same bound)."""
    g = torch.Generator(device=dev).manual_seed(77)
    return [{k: ((torch.rand(v.shape, generator=g, device=dev) * 2 - 1) * float(v.float().abs().max())).to(v.dtype) for k, v in own.items()}
            for _ in range(n)]


def leg(model, cfg_d, B, samples, ids, dev):
    n_codes = cfg_d["audio_card"] - 2
    gen = GPTGen(model, use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25, n_audio_codes=n_codes)
    g = torch.Generator(device=dev).manual_seed(1234)
    prompt = torch.randint(0, n_codes, (B, cfg_d["n_q"] + 1, 8), generator=g, device=dev)
    torch.manual_seed(1234)
    gen.begin(B, adapter_ids=ids)
    try:
        gen.set_blanking([False] + [True] * (cfg_d["dep_q"] - 1))
        h, logits = gen.prefill(prompt)
        gen.start(h, logits)
        for _ in range(WARMUP):
            gen.step()
        bench._quiesce_host()
        return bench._timing(bench._sample_steps(lambda i: gen.step(), samples))["median_ms"]
    finally:
        gen.end()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--lm-config", choices=["qwen0.5b", "tiny"], default="qwen0.5b")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lora_bank_ab.json"))
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats: at least 7 (the figures are medians over the rounds)")
    B = a.batch
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg_d = dict(synth.GPT_QWEN_0_5B if a.lm_config != "tiny" else synth.GPT_TINY_GQA)
    cfg = Config.from_dict(cfg_d)
    sd = synth.gpt_state_dict(cfg_d, seed=0, device=str(dev))
    base = {k: v for k, v in sd.items() if not is_lora(k)}
    own = {k: v for k, v in sd.items() if is_lora(k)}
    merged = GPT.from_state_dict(dict(sd), cfg)
    unmerged = GPT.from_state_dict(dict(sd), cfg, merge_lora=False)                   # (shares the dense tensors with `base`)
    sets = random_sets(own, B, dev)
    bank4 = GPT.from_state_dict(dict(base), cfg, merge_lora=False)
    bank4.load_adapter_bank(sets[:4])
    bankB = GPT.from_state_dict(dict(base), cfg, merge_lora=False)
    bankB.load_adapter_bank(sets)
    bank_bytes = sum(A.numel() * 2 + Bm.numel() * 2 for A, Bm, _ in bankB.adapter_bank().values())
    del sets
    legs = {"merged": (merged, None), "unmerged": (unmerged, None), "bank_1of4": (bank4, [1] * B),
            "bank_32": (bankB, list(range(B))), "bank_none": (bankB, [-1] * B)}
    rounds = []
    for _ in range(a.repeats):
        rounds.append({k: leg(m, cfg_d, B, a.samples, ids, dev) for k, (m, ids) in legs.items()})
    med = {k: round(statistics.median(r[k] for r in rounds), 4) for k in legs}
    out = {"tool": "tools/bench_lora_bank.py", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(dev), "lm_config": a.lm_config,
           "batch": B, "lora_r": cfg_d["lora_r"], "samples_per_leg": a.samples, "repeats": a.repeats,
           "bank_bytes_per_set": bank_bytes // B,
           "method": "ms per frame: median of individually synchronised graph-replayed GPTGen.step frames (bench.py `timing`) per leg, "
                     "median over the rounds; legs interleaved (merged, unmerged, bank_1of4, bank_32, bank_none) in one process",
           "median_ms": med, "rounds_ms": rounds,
           "bank_1of4_over_unmerged": round(med["bank_1of4"] / med["unmerged"], 4),
           "bank_32_over_merged": round(med["bank_32"] / med["merged"], 4),
           "bank_none_over_merged": round(med["bank_none"] / med["merged"], 4),
           "unmerged_over_merged": round(med["unmerged"] / med["merged"], 4)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
