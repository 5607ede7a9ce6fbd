"""A/B of the LM frame with bf16 and with fp8 (e4m3, weight-only) weight storage: one process, one box, alternating.

    python tools/bench_lm_fp8w.py [--rounds 2] [--samples 60] [--lm-config moshi7b|tiny] [--batch B]

Prints ONE JSON line: ``lm_b1`` (LMGen.step), ``lm_ctx3000`` (the same with the temporal rings 3000 frames full) and ``e2e_b1`` (Mimi encode ->
LMGen -> Mimi decode, StreamingPipeline), each as ms per frame -- the median of ``--samples`` individually synchronised frames, bench.py's
``timing`` -- for bf16 and fp8, and the ratio fp8 / bf16.

Order: the bf16 model as built (``bf16_before``: exactly what bench.py measures), then ``quantize_weights_("fp8")`` and ``--rounds`` times
(fp8, bf16).  Quantisation overwrites the bf16 parameters with the dequantised values, so the later bf16 legs run the untouched bf16
code path (persistent temporal launch at the full ring included) on those values by switching the model's ``weight_dtype`` mark back
for the leg -- same kernels, same bytes as ``bf16_before``, which the line reports next to them.  The ratio is median(fp8 legs) /
median(bf16 legs after quantisation), legs interleaved.

``--batch B`` (B > 1): the same for B streams -- ``lm_b{B}`` (LMGen.step on B streams) and ``e2e_b{B}`` (StreamingPipeline at B
streams); above two rows the fp8 legs run the weight-only fp8 skinny GEMM (``ops.gemm_skinny_fp8w``), the bf16 legs the bf16 skinny
GEMM.  There is no full-ring leg at B > 1."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from rstnet_amd import _lib, synth  # noqa: E402
from rstnet_amd.codec.mimi import MimiCodec  # noqa: E402
from rstnet_amd.lm.model import LMGen  # noqa: E402
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
    ap.add_argument("--batch", type=int, default=1, help="streams per frame; above 1 the legs are lm_b{B} and e2e_b{B}")
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
        model.weight_dtype = model.transformer.weight_dtype = dtype

    def run_all():
        bench._quiesce_host()
        return {k: fn() for k, fn in legs.items()}

    before = run_all()
    model.quantize_weights_("fp8")
    runs = {"fp8": [], "bf16": []}
    for _ in range(a.rounds):
        for dtype in ("fp8", "bf16"):
            mark(dtype)
            runs[dtype].append(run_all())
    mark("fp8")
    out = {"tool": "tools/bench_lm_fp8w.py", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(dev), "lm_config": a.lm_config,
           "params": n_params, "samples_per_leg": a.samples, "rounds": a.rounds, **({"batch": B} if B > 1 else {}),
           "method": "ms per frame: median of individually synchronised frames (bench.py `timing`); legs interleaved fp8 / bf16 in one process"}
    for k in legs:
        f8 = statistics.median(r[k] for r in runs["fp8"])
        b16 = statistics.median(r[k] for r in runs["bf16"])
        out[k] = {"bf16_before_ms": before[k], "bf16_ms": round(b16, 4), "fp8_ms": round(f8, 4), "ratio_fp8_over_bf16": round(f8 / b16, 4),
                  "bf16_legs_ms": [r[k] for r in runs["bf16"]], "fp8_legs_ms": [r[k] for r in runs["fp8"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
