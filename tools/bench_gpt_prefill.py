"""The multi-position pass of `GPT` on bf16 rings (`lm_attn_prefill(heads=H)` + `lm_ring_append`) against the fp32-ring route it
had before (`lm_rope_append` + `attention`), and the graph-replayed T = 1 step on a full ring with fp32 against bf16 rings -- at
`GPT_QWEN_0_5B` (MHA, 16 heads of 64) and at the same shape with `n_head=14, n_query_groups=2, n_embd=896` (GQA 7:1), one process.

    python tools/bench_gpt_prefill.py [--repeats 5] [--samples 40] [--lengths 256,1024] [--batches 1,32] [--config qwen|tiny] [--out profiles/gpt_prefill.json]

Writes ONE JSON object (and prints it as one line).  Per shape:

  * ``prompt[B][T]``: `GPTGen.prefill` of T positions into a fresh session (ring of context + 1 slots) -- device events around the
    call, one warm-up call first; ``fp32_ms`` is the route every prompt took before (fp32 rings), ``bf16_ms`` the new route;
  * ``attention[B][T]``: the attention + append launches of ONE block alone, on an empty ring, same two routes;
  * ``step[B]``: the median graph-replayed `forward_global` T = 1 step on a ring holding 3000 positions, fp32 against bf16 rings.

The baseline of every ratio is the fp32 route timed in this very process, never a number from the new route.  No hard condition: the
tool reports."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from rstnet_amd import _lib, ops, synth  # noqa: E402
from rstnet_amd.lm.generate import GPTGen  # noqa: E402
from rstnet_amd.lm.gpt import GPT, Config, prefill_window  # noqa: E402
from rstnet_amd.lm.model import PREFILL_CHUNK  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
NAMES = {F32: "fp32", BF16: "bf16"}


def _events_ms(fn, repeats, before=None):
    out = []
    for _ in range(repeats):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def _prompt(cfg, B, T, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    text = torch.randint(0, cfg["padded_vocab_size"], (B, 1, T), generator=g, device=dev)
    audio = torch.randint(0, cfg["audio_card"], (B, cfg["n_q"], T), generator=g, device=dev)
    return torch.cat([text, audio], 1)


def prompt_leg(cfg, model, dev, B, T, kv, repeats):
    """`GPTGen.prefill` of T positions at position 0 of a fresh ring, every timed call (the counters are rewound between calls)."""
    gen = GPTGen(model, use_sampling=False)
    toks = _prompt(cfg, B, T, dev, 100 + T)
    gen.begin(B, kv_dtype=kv)
    try:
        st = model.transformer._streaming_state
        gen.prefill(toks)                                        # warm-up: every shape of the timed calls
        ms = _events_ms(lambda: gen.prefill(toks), repeats, before=st.reset)
    finally:
        gen.end()
    return round(statistics.median(ms), 4)


def attention_leg(cfg, dev, B, T, kv, repeats):
    """The attention + append launches of one block on an empty ring of context + 1 slots."""
    c = Config.from_dict(cfg)
    H, G, D, n, cap = c.n_head, c.n_query_groups, c.head_size, c.rope_n_elem, c.context + 1
    g = torch.Generator(device=dev).manual_seed(7)
    kc, vc = torch.zeros(B, G, cap, D, device=dev, dtype=kv), torch.zeros(B, G, cap, D, device=dev, dtype=kv)
    qkv = torch.randn(B, T, (H + 2 * G) * D, generator=g, device=dev)
    pos = torch.zeros(1, device=dev, dtype=torch.long)
    base = float(c.rope_base)
    if kv == F32:
        def fn():
            q = ops.lm_rope_append(qkv, kc, vc, pos, heads=H, rope=True, max_period=base, rope_dims=n)
            ops.attention(q, kc, vc, pos_dev=pos, ring=True, context=c.context)
    else:
        freqs, window = ops.gpt_rope_freqs(dev, base, n), prefill_window(c.context, cap)
        parts = [(t0, qkv[:, t0:t0 + PREFILL_CHUNK].contiguous()) for t0 in range(0, T, PREFILL_CHUNK)]      # (the chunks `run` forms)

        def fn():
            for t0, part in parts:
                pos.fill_(t0)
                ops.lm_attn_prefill(part, kc, vc, pos, window=window, rope=True, max_period=base, rope_dims=n, heads=H, freqs=freqs)
                ops.lm_ring_append(part, kc, vc, pos, rope=True, max_period=base, rope_dims=n, heads=H, freqs=freqs)
            pos.zero_()
    fn()
    return round(1e3 * statistics.median(_events_ms(fn, repeats)), 2)


def step_leg(cfg, model, dev, B, kv, samples, filled):
    """Graph-replayed T = 1 steps of a `streaming(B)` session whose ring of `context` slots holds `filled` positions."""
    col = _prompt(cfg, B, 1, dev, 5)
    saved = model.kv_dtype
    model.kv_dtype = kv
    try:
        with model.streaming(B):
            st = model.transformer._streaming_state
            g = torch.Generator(device=dev).manual_seed(11)
            for t in st.k + st.v:
                t.copy_((0.5 * torch.randn(t.shape, generator=g, device=dev)).to(kv))
            st.pos.fill_(filled)
            st.offset_cpu = filled
            for _ in range(6):                                   # warm-up, capture, replays
                model.forward_global(col)
            return bench._timing(bench._sample_steps(lambda i: model.forward_global(col), samples))
    finally:
        model.kv_dtype = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--lengths", default="256,1024")
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--config", choices=["qwen", "tiny"], default="qwen")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt_prefill.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_gpt_prefill.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if a.config == "qwen":
        shapes = {"mha_16x64": dict(synth.GPT_QWEN_0_5B), "gqa_14_over_2": dict(synth.GPT_QWEN_0_5B, n_head=14, n_query_groups=2, n_embd=896)}
        filled = 3000
    else:       # (a dry run of the tool itself; the ring must hold more than 64 slots for bf16)
        shapes = {"tiny_gqa": dict(synth.GPT_TINY_GQA, context=400, block_size=4096)}
        filled = 400
    lengths, batches = [int(x) for x in a.lengths.split(",")], [int(x) for x in a.batches.split(",")]
    out = {"tool": "tools/bench_gpt_prefill.py", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(dev), "chunk": PREFILL_CHUNK,
           "method": "prompt / attention: median of device-event intervals after one warm-up call per shape; step: median of individually "
                     "synchronised graph replays (bench.py `timing`); every ratio is bf16 route / fp32 route of this process",
           "shapes": {}}
    for name, cfg in shapes.items():
        model = GPT.from_state_dict(synth.gpt_state_dict(cfg, seed=0, device=str(dev)), Config.from_dict(cfg))
        r = {"config": {k: cfg[k] for k in ("n_layer", "n_embd", "n_head", "n_query_groups", "context")}, "prompt": {}, "attention": {}, "step": {}}
        for B in batches:
            r["prompt"][str(B)], r["attention"][str(B)] = {}, {}
            for T in lengths:
                bench._quiesce_host()
                f, b = (prompt_leg(cfg, model, dev, B, T, kv, a.repeats) for kv in (F32, BF16))
                r["prompt"][str(B)][str(T)] = {"fp32_ms": f, "bf16_ms": b, "ratio_bf16_over_fp32": round(b / f, 4)}
                f, b = (attention_leg(cfg, dev, B, T, kv, 4 * a.repeats) for kv in (F32, BF16))
                r["attention"][str(B)][str(T)] = {"fp32_us": f, "bf16_us": b, "ratio_bf16_over_fp32": round(b / f, 4)}
            bench._quiesce_host()
            f, b = (step_leg(cfg, model, dev, B, kv, a.samples, filled) for kv in (F32, BF16))
            r["step"][str(B)] = {"ring_positions": filled, "fp32_ms": f["median_ms"], "bf16_ms": b["median_ms"],
                                 "ratio_bf16_over_fp32": round(b["median_ms"] / f["median_ms"], 4), "fp32_timing": f, "bf16_timing": b}
        out["shapes"][name] = r
        del model
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
