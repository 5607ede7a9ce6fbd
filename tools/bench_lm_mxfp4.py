"""A/B/C of the batch-1 LM frame with bf16, fp8 (e4m3) and MXFP4 weight-only storage: one process, one box, legs interleaved.

    python tools/bench_lm_mxfp4.py [--rounds 2] [--samples 60] [--lm-config moshi7b|tiny] [--batch B]

Prints ONE JSON line: ``lm_b1`` (LMGen.step), ``lm_ctx3000`` (the same with the temporal rings 3000 frames full) and ``e2e_b1`` (Mimi encode ->
LMGen -> Mimi decode, StreamingPipeline), each as ms per frame -- the median of ``--samples`` individually synchronised frames, bench.py's
``timing`` -- for bf16, fp8 and mxfp4, and the ratios mxfp4 / bf16 and mxfp4 / fp8.

Order: the bf16 model as built (``bf16_before``: exactly what bench.py measures), then ``quantize_weights_("mxfp4")`` and ``--rounds`` times
(bf16, fp8, mxfp4).  Time does not depend on weight values, so ONE model serves all three legs: after quantisation the per-layer
matrices also get fp8 copies of their (already rounded) values through the private ``_attach_copy`` -- the public API never holds both
kinds for one matrix -- and a leg switches the model's ``weight_dtype`` mark: ``"bf16"`` runs the untouched bf16 code path (persistent
temporal launch at the full ring included), ``"fp8"`` streams fp8 copies of every covered matrix exactly as an fp8 model does,
``"mxfp4"`` the MXFP4 copies of the per-layer matrices and fp8 heads.  Every ratio's baseline is a leg of the same process.

``--batch B`` (B > 1): the same for B streams -- ``lm_b{B}`` (LMGen.step on B streams) and ``e2e_b{B}`` (StreamingPipeline at B streams),
no full-ring leg -- with FOUR legs per round: bf16, fp8 (``ops.gemm_skinny_fp8w``), ``mxfp4`` (the model of plain
``quantize_weights_("mxfp4")``: above two rows its per-layer matrices are read as bf16) and ``mxfp4_batched`` (the same model after
``quantize_weights_("mxfp4", batched=True)``: ``ops.gemm_skinny_mxfp4w``), the last two by switching the model's ``mxfp4_batched`` flag.
Ratios: mxfp4_batched / mxfp4 (what opting in changes), mxfp4_batched / fp8 and mxfp4_batched / bf16."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from rstnet_amd import _lib, ops, synth  # noqa: E402
from rstnet_amd.codec.mimi import MimiCodec  # noqa: E402
from rstnet_amd.lm.model import LMGen, _attach_copy, _w8  # noqa: E402
from rstnet_amd.pipeline import StreamingPipeline  # noqa: E402

WARMUP = 12


def lm_leg(cfg, model, dev, samples, context, B=1):
    gen = LMGen(model, use_sampling=True, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25)
    g = torch.Generator(device=dev).manual_seed(1234)
    user = torch.randint(0, cfg["card"], (WARMUP + samples, B, cfg["n_q"] - cfg["dep_q"], 1), generator=g, device=dev)
    torch.manual_seed(1234)
    with gen.streaming(B):
        if context:
            st = model.transformer._streaming_state
            st.pos.fill_(context)
            st.offset_cpu = context
        for i in range(WARMUP):
            gen.step(user[i])
        return bench._timing(bench._sample_steps(lambda i: gen.step(user[WARMUP + i]), samples))["median_ms"]


def e2e_leg(cfg, model, mimi, dev, samples, B=1):
    gen = LMGen(model, use_sampling=True)
    pcm = synth.synth_audio(B, 1920 * (WARMUP + samples), seed=200).to(dev)
    torch.manual_seed(1234)
    with StreamingPipeline(mimi, gen, B) as pipe:
        step = lambda s: pipe.step(pcm[:, :, s * 1920:(s + 1) * 1920].contiguous())     # noqa: E731
        for i in range(WARMUP):
            step(i)
        return bench._timing(bench._sample_steps(lambda i: step(WARMUP + i), samples))["median_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--samples", type=int, default=60)
    ap.add_argument("--lm-config", choices=["moshi7b", "tiny"], default="moshi7b")
    ap.add_argument("--batch", type=int, default=1, help="streams per frame; above 1 the legs are lm_b{B} and e2e_b{B}, with the batched MXFP4 route as a fourth storage leg")
    ap.add_argument("--legs", default=None, help="comma-separated subset (default: all legs of the batch size)")
    a = ap.parse_args()
    B = a.batch
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg, model, n_params = bench.build_lm(argparse.Namespace(lm_config=a.lm_config, kv_dtype="bf16"), 0, 1, dev)
    if a.lm_config == "tiny":
        cfg = dict(synth.LM_TINY_16Q)
        from rstnet_amd.lm.model import LMModel
        model = LMModel.from_state_dict(synth.lm_state_dict(cfg, seed=0, device=str(dev)), cfg)
    mimi = MimiCodec.from_state_dict(synth.mimi_state_dict(0)).to(dev)
    legs = {f"lm_b{B}": lambda: lm_leg(cfg, model, dev, a.samples, 0, B)}
    if B == 1:
        legs["lm_ctx3000"] = lambda: lm_leg(cfg, model, dev, a.samples, 3000)
    legs[f"e2e_b{B}"] = lambda: e2e_leg(cfg, model, mimi, dev, a.samples, B)
    if a.legs:
        legs = {k: v for k, v in legs.items() if k in a.legs.split(",")}

    def mark(dtype):
        model.weight_dtype = model.transformer.weight_dtype = dtype.split("_")[0]
        model.mxfp4_batched = model.transformer.mxfp4_batched = dtype == "mxfp4_batched"

    def run_all():
        bench._quiesce_host()
        return {k: fn() for k, fn in legs.items()}

    before = run_all()
    model.quantize_weights_("mxfp4")
    with torch.no_grad():
        for mod, name in model._layer_weights():          # fp8 copies next to the MXFP4 ones, for the fp8 legs only
            if _w8(mod, name) is None:
                _attach_copy(mod, name, "8", *ops.quantize_rows_fp8(getattr(mod, name).detach()))
    order = ("bf16", "fp8", "mxfp4") + (("mxfp4_batched",) if B > 1 else ())
    runs = {d: [] for d in order}
    for _ in range(a.rounds):
        for dtype in order:
            mark(dtype)
            runs[dtype].append(run_all())
    mark("mxfp4")
    out = {"tool": "tools/bench_lm_mxfp4.py", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(dev), "lm_config": a.lm_config,
           "params": n_params, "samples_per_leg": a.samples, "rounds": a.rounds, **({"batch": B} if B > 1 else {}),
           "method": "ms per frame: median of individually synchronised frames (bench.py `timing`); legs interleaved " + " / ".join(order) + " in "
                     "one process on one model (weight_dtype mark switched per leg)"}
    for k in legs:
        med = {d: statistics.median(r[k] for r in runs[d]) for d in order}
        out[k] = {"bf16_before_ms": before[k], "bf16_ms": round(med["bf16"], 4), "fp8_ms": round(med["fp8"], 4),
                  "mxfp4_ms": round(med["mxfp4"], 4), "ratio_mxfp4_over_bf16": round(med["mxfp4"] / med["bf16"], 4),
                  "ratio_mxfp4_over_fp8": round(med["mxfp4"] / med["fp8"], 4), "ratio_fp8_over_bf16": round(med["fp8"] / med["bf16"], 4),
                  "bf16_legs_ms": [r[k] for r in runs["bf16"]], "fp8_legs_ms": [r[k] for r in runs["fp8"]],
                  "mxfp4_legs_ms": [r[k] for r in runs["mxfp4"]]}
        if B > 1:
            nb = med["mxfp4_batched"]
            out[k].update({"mxfp4_batched_ms": round(nb, 4), "ratio_mxfp4_batched_over_mxfp4": round(nb / med["mxfp4"], 4),
                           "ratio_mxfp4_batched_over_fp8": round(nb / med["fp8"], 4), "ratio_mxfp4_batched_over_bf16": round(nb / med["bf16"], 4),
                           "mxfp4_batched_legs_ms": [r[k] for r in runs["mxfp4_batched"]]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
