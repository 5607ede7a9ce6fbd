"""`LMGen.prefill` against replaying the same frames through `LMGen.step`, at the Moshi-7B shape, batch 1, one process.

    python tools/bench_lm_prefill.py [--samples 60] [--repeats 5] [--lengths 64,256,1024] [--lm-config moshi7b|tiny] [--out profiles/lm_prefill.json]
                                     [--fp8 | --mxfp4]

Writes ONE JSON object (and prints it as one line):

  * ``step_ms``: the median `LMGen.step` frame (bench.py's `timing`: host clock around individually synchronised frames, after warm-up);
  * ``prefill[T]``: `LMGen.prefill` of T frames -- device events around the call (token bookkeeping, embedding, the whole launch chain),
    one warm-up call of the same length first, then ``--repeats`` timed calls in ONE session, so that the later ones run on a fuller ring
    than the baseline step ever sees; ``baseline_ms = T * step_ms`` is what replaying costs, never a number from the prefill path;
  * ``attention``: `ops.lm_attn_prefill` (its staging launch and its attention launch) and `ops.lm_ring_append` alone, per layer, at the
    temporal shape (32 heads of 128, bf16 ring of 3000 slots), on an empty ring and on a full one;
  * ``--fp8``: ``prefill_fp8w[T]``, after everything above: the model is quantised (``quantize_weights_("fp8")``) and every length runs
    twice as (fp8, bf16) -- the bf16 legs by switching the ``weight_dtype`` mark on the same model, so both stream the same values;
    ``ratio_fp8_over_bf16`` compares the two medians of this process (the 64-row chunks run ``ops.gemm_skinny_fp8w`` against
    ``ops.gemm_skinny``);
  * ``--mxfp4`` (instead of ``--fp8``: a model is quantised to one format): ``prefill_mxfp4w[T]``, after everything above: the model is
    quantised (``quantize_weights_("mxfp4")``), its per-layer matrices also get fp8 copies of the rounded values (tools/bench_lm_mxfp4.py)
    and every length runs twice as (mxfp4_batched, mxfp4, fp8, bf16) by switching the model's marks: ``mxfp4_batched`` streams the MXFP4
    copies in the 64-row chunks (``ops.gemm_skinny_mxfp4w``), ``mxfp4`` reads those matrices as bf16 there (the route without the opt-in);
    ratios of the first against each of the others.

Exit status 1 when a 256-frame prefill is not under 1/8 of its baseline: the linears then stream the temporal weights 4 times instead of
256 times and the depth phase is gone, so missing that means a route is wrong, not slow."""
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
from rstnet_amd.lm.model import PREFILL_CHUNK, LMGen  # noqa: E402

WARMUP = 12


def _events_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def step_leg(cfg, model, dev, samples):
    gen = LMGen(model, use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25)
    g = torch.Generator(device=dev).manual_seed(1234)
    user = torch.randint(0, cfg["card"], (WARMUP + samples, 1, cfg["n_q"] - cfg["dep_q"], 1), generator=g, device=dev)
    torch.manual_seed(1234)
    with gen.streaming(1):
        for i in range(WARMUP):
            gen.step(user[i])
        return bench._timing(bench._sample_steps(lambda i: gen.step(user[WARMUP + i]), samples))


def prefill_leg(cfg, model, dev, T, repeats):
    gen = LMGen(model, use_sampling=True)
    g = torch.Generator(device=dev).manual_seed(4321 + T)
    user = torch.randint(0, cfg["card"], (1, cfg["n_q"] - cfg["dep_q"], T), generator=g, device=dev)
    own = torch.randint(0, cfg["card"], (1, cfg["dep_q"] + 1, T), generator=g, device=dev)
    own[:, 0] = torch.randint(0, cfg["text_card"], (1, T), generator=g, device=dev)
    with gen.streaming(1):
        gen.prefill(user, own)                                   # warm-up: every shape of the timed calls
        ms = _events_ms(lambda: gen.prefill(user, own), repeats)
        assert gen._streaming_state.offset == (repeats + 1) * T
    return {"frames": T, "ms": round(statistics.median(ms), 4), "samples_ms": [round(x, 4) for x in ms],
            "positions": f"{T} .. {(repeats + 1) * T - 1}"}


def attention_leg(cfg, dev, Tc, pos0, repeats):
    H, D, cap = cfg["num_heads"], cfg["dim"] // cfg["num_heads"], cfg["context"]
    g = torch.Generator(device=dev).manual_seed(7)
    kc = (0.5 * torch.randn(1, H, cap, D, generator=g, device=dev)).to(torch.bfloat16)
    vc = (0.5 * torch.randn(1, H, cap, D, generator=g, device=dev)).to(torch.bfloat16)
    qkv = torch.randn(1, Tc, 3 * H * D, generator=g, device=dev)
    pos = torch.full((1,), pos0, device=dev, dtype=torch.long)
    window = min(cfg["context"], cap - 1)
    att = lambda: ops.lm_attn_prefill(qkv, kc, vc, pos, window=window, rope=True, max_period=cfg["max_period"])      # noqa: E731
    app = lambda: ops.lm_ring_append(qkv, kc, vc, pos, rope=True, max_period=cfg["max_period"])                       # noqa: E731
    for _ in range(3):
        att(), app()
    return {"Tc": Tc, "pos": pos0, "attn_prefill_us": round(1e3 * statistics.median(_events_ms(att, repeats)), 2),
            "ring_append_us": round(1e3 * statistics.median(_events_ms(app, repeats)), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lengths", default="64,256,1024")
    ap.add_argument("--lm-config", choices=["moshi7b", "tiny"], default="moshi7b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_prefill.json"))
    ap.add_argument("--fp8", action="store_true", help="add the quantised legs (prefill_fp8w), fp8 / bf16 interleaved on the same model")
    ap.add_argument("--mxfp4", action="store_true", help="add the MXFP4 legs (prefill_mxfp4w): batched route / bf16 batched route / fp8 / bf16 interleaved on one model")
    a = ap.parse_args()
    if a.fp8 and a.mxfp4:
        ap.error("--fp8 and --mxfp4 exclude each other: a model is quantised to one format")
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_lm_prefill.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg, model, n_params = bench.build_lm(argparse.Namespace(lm_config=a.lm_config, kv_dtype="bf16"), 0, 1, dev)
    if a.lm_config == "tiny":
        cfg = dict(synth.LM_TINY_16Q)
        from rstnet_amd.lm.model import LMModel
        model = LMModel.from_state_dict(synth.lm_state_dict(cfg, seed=0, device=str(dev)), cfg)
    bench._quiesce_host()
    step = step_leg(cfg, model, dev, a.samples)
    out = {"tool": "tools/bench_lm_prefill.py", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(dev), "lm_config": a.lm_config,
           "params": n_params, "batch": 1, "chunk": PREFILL_CHUNK, "step_ms": step["median_ms"], "step_timing": step,
           "method": "step: median of individually synchronised frames (bench.py `timing`); prefill / kernels: median of device-event "
                     "intervals after one warm-up call per shape; one process; box-to-box spread of such numbers is about +-3 %",
           "prefill": {}, "attention": []}
    for T in [int(x) for x in a.lengths.split(",")]:
        bench._quiesce_host()
        r = prefill_leg(cfg, model, dev, T, a.repeats)
        r["baseline_ms"] = round(T * step["median_ms"], 3)
        r["ratio_prefill_over_baseline"] = round(r["ms"] / r["baseline_ms"], 5)
        r["us_per_frame"] = round(1e3 * r["ms"] / T, 2)
        out["prefill"][str(T)] = r
    if a.lm_config == "moshi7b":
        for Tc, pos0 in ((64, 0), (256, 0), (64, 3000), (256, 3000)):
            out["attention"].append(attention_leg(cfg, dev, Tc, pos0, 20))
    if a.fp8:
        model.quantize_weights_("fp8")
        out["prefill_fp8w"] = {}
        for T in [int(x) for x in a.lengths.split(",")]:
            ms = {"fp8": [], "bf16": []}
            for _ in range(2):
                for dtype in ("fp8", "bf16"):
                    model.weight_dtype = model.transformer.weight_dtype = dtype
                    bench._quiesce_host()
                    ms[dtype].append(prefill_leg(cfg, model, dev, T, a.repeats)["ms"])
            model.weight_dtype = model.transformer.weight_dtype = "fp8"
            f8, b16 = statistics.median(ms["fp8"]), statistics.median(ms["bf16"])
            out["prefill_fp8w"][str(T)] = {"frames": T, "fp8_ms": round(f8, 4), "bf16_ms": round(b16, 4), "ratio_fp8_over_bf16": round(f8 / b16, 4),
                                           "fp8_legs_ms": ms["fp8"], "bf16_legs_ms": ms["bf16"]}
    if a.mxfp4:
        from rstnet_amd.lm.model import _attach_copy, _w8
        model.quantize_weights_("mxfp4", batched=True)
        with torch.no_grad():
            for mod, name in model._layer_weights():          # fp8 copies next to the MXFP4 ones, for the fp8 legs only
                if _w8(mod, name) is None:
                    _attach_copy(mod, name, "8", *ops.quantize_rows_fp8(getattr(mod, name).detach()))

        def mark(leg):
            model.weight_dtype = model.transformer.weight_dtype = leg.split("_")[0]
            model.mxfp4_batched = model.transformer.mxfp4_batched = leg == "mxfp4_batched"
        order = ("mxfp4_batched", "mxfp4", "fp8", "bf16")
        out["prefill_mxfp4w"] = {}
        for T in [int(x) for x in a.lengths.split(",")]:
            ms = {leg: [] for leg in order}
            for _ in range(2):
                for leg in order:
                    mark(leg)
                    bench._quiesce_host()
                    ms[leg].append(prefill_leg(cfg, model, dev, T, a.repeats)["ms"])
            mark("mxfp4_batched")
            med = {leg: statistics.median(ms[leg]) for leg in order}
            out["prefill_mxfp4w"][str(T)] = {"frames": T, **{leg + "_ms": round(med[leg], 4) for leg in order},
                                             **{"ratio_mxfp4_batched_over_" + leg: round(med["mxfp4_batched"] / med[leg], 4) for leg in order[1:]},
                                             **{leg + "_legs_ms": ms[leg] for leg in order}}
    gate = out["prefill"].get("256")
    if gate is not None:
        out["hard_condition"] = {"what": "prefill of 256 frames < 1/8 of 256 x step", "holds": bool(gate["ms"] < gate["baseline_ms"] / 8)}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if gate is not None and not out["hard_condition"]["holds"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
