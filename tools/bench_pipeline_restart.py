"""What per-stream sessions cost, at the `e2e_b32` shape (32 streams, one frame graph per 80 ms frame):

  (a) the scalar pipeline frame against the per-stream pipeline frame -- one process, one model, the two sessions measured in turns;
  (b) one `StreamingPipeline.reset_streams([b])` between two frames (host time until the reset's writes have completed);
  (c) the scalar frame on THIS library against another build of it (`--parent-lib`: the parent commit's librstnet_hip.so) through
      `tools/ab.py LIB=`, in alternating child processes (`bench.py --workload e2e --lm-batch 32`).

Medians of `--rounds` (7) rounds; every round measures each leg once, in alternating order.  For (c) the spread max / min of the
same-library samples of this very run is recorded next to the ratio: a ratio inside it is not a difference this run can show.

    python tools/bench_pipeline_restart.py --parent-lib /path/to/parent/librstnet_hip.so --out profiles/pipeline_per_stream.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ms_per_frame(pipe, pcm, first, frames):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(first, first + frames):
        pipe.step(pcm[:, :, s * 1920:(s + 1) * 1920].contiguous())
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / frames * 1e3


def in_process(args):
    """(a) and (b): both sessions stay open (each owns its states; the model's weights are shared) and take turns."""
    import torch
    from rstnet_amd import _lib, synth
    from rstnet_amd.codec.mimi import MimiCodec
    from rstnet_amd.lm.model import LMGen, LMModel
    from rstnet_amd.pipeline import StreamingPipeline
    dev = torch.device("cuda:0")
    B = args.batch
    cfg = dict(synth.LM_MOSHI_7B if args.lm_config == "moshi7b" else synth.LM_TINY)
    # two models on the same weight tensors: a model's streaming state belongs to one live session
    sd = synth.lm_state_dict(cfg, seed=0, device=str(dev))
    models = [LMModel.from_state_dict(sd, cfg) for _ in range(2)]
    mimi_sd = synth.mimi_state_dict(0)
    mimis = [MimiCodec.from_state_dict(mimi_sd).to(dev) for _ in range(2)]
    total = args.warmup + args.rounds * args.frames + args.rounds * 2 + 4
    pcm = synth.synth_audio(B, 1920 * total, seed=200).to(dev)
    torch.manual_seed(1234)
    legs = {"scalar": [], "per_stream": []}
    resets = []
    with StreamingPipeline(mimis[0], LMGen(models[0]), B) as scalar, \
            StreamingPipeline(mimis[1], LMGen(models[1]), B, per_stream=True) as per_stream:
        pipes = {"scalar": scalar, "per_stream": per_stream}
        at = {"scalar": 0, "per_stream": 0}
        for name, pipe in pipes.items():
            _ms_per_frame(pipe, pcm, 0, args.warmup)
            at[name] = args.warmup
        for r in range(args.rounds):
            for name in (("scalar", "per_stream") if r % 2 == 0 else ("per_stream", "scalar")):
                legs[name].append(_ms_per_frame(pipes[name], pcm, at[name], args.frames))
                at[name] += args.frames
            # (b): one row restarts between two frames; the frames around it keep the session going
            row = r % B
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            per_stream.reset_streams([row])
            torch.cuda.synchronize()
            resets.append((time.perf_counter() - t0) * 1e3)
            _ms_per_frame(per_stream, pcm, at["per_stream"], 2)
            at["per_stream"] += 2
        graph_kept = per_stream._fused is not None and per_stream._fused.calls == 1
    med = {k: statistics.median(v) for k, v in legs.items()}
    return {"build_id": _lib.build_id(), "streams": B, "lm_config": args.lm_config, "frames_per_sample": args.frames, "rounds": args.rounds,
            "scalar_ms_per_frame": {"median": round(med["scalar"], 4), "samples": [round(v, 4) for v in legs["scalar"]]},
            "per_stream_ms_per_frame": {"median": round(med["per_stream"], 4), "samples": [round(v, 4) for v in legs["per_stream"]]},
            "per_stream_over_scalar": round(med["per_stream"] / med["scalar"], 4),
            "reset_one_row_ms": {"median": round(statistics.median(resets), 4), "samples": [round(v, 4) for v in resets]},
            "frame_graph_never_recaptured": bool(graph_kept)}


def _child(args, lib):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ab.py")] + ([f"LIB={lib}"] if lib else []) + [
        "--", "--workload", "e2e", "--lm-batch", str(args.batch), "--lm-config", args.lm_config, "--steps", str(args.frames), "--warmup",
        str(args.warmup), "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.child_timeout)
    if out.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({out.returncode}): {out.stderr[-2000:]}")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def against_parent(args):
    """(c): this library and the parent's in alternating child processes, the scalar `e2e_b32` frame of bench.py."""
    if not args.parent_lib:
        return {"skipped": "no --parent-lib given"}
    legs = {"this": [], "parent": []}
    for r in range(args.rounds):
        for name in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            legs[name].append(_child(args, args.parent_lib if name == "parent" else None))
    med = {k: statistics.median(v) for k, v in legs.items()}
    spread = {k: max(v) / min(v) for k, v in legs.items()}
    ratio = med["this"] / med["parent"]
    box = max(spread.values())
    return {"this_ms_per_frame": {"median": round(med["this"], 4), "samples": legs["this"]},
            "parent_ms_per_frame": {"median": round(med["parent"], 4), "samples": legs["parent"]},
            "this_over_parent": round(ratio, 4), "same_library_spread_max_over_min": {k: round(v, 4) for k, v in spread.items()},
            "ratio_inside_same_library_spread": bool(1.0 / box <= ratio <= box)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lm-config", choices=["moshi7b", "tiny"], default="moshi7b")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40, help="timed frames per sample")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's librstnet_hip.so (leg c); without it (c) is skipped")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--skip-in-process", action="store_true")
    ap.add_argument("--out", default=None, help="write the result here as JSON (it is always printed as one line)")
    args = ap.parse_args()
    # (c) first: its children must have the GPU's memory to themselves (the 7B model twice does not fit next to a third copy's captures)
    result = {"shape": "e2e_b32" if args.batch == 32 and args.lm_config == "moshi7b" else f"e2e_b{args.batch}_{args.lm_config}",
              "against_parent": against_parent(args)}
    if not args.skip_in_process:
        result.update(in_process(args))
    result["note"] = "one machine, one run: figures move by about +-3 % from box to box"
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
