"""What per-stream sampling costs, at the `e2e_b32` shape (32 streams, one frame graph per 80 ms frame):

  (a) the per-stream pipeline frame with scalar sampling against the same frame with `LMGen(per_stream_sampling=True)` -- one process, one
      set of weights, the two sessions measured in turns;
  (b) the noise launch alone (`ops.noise_exp_rows` at the frame's shape, [32, top_k_text + dep_q * top_k]) under HIP events;
  (c) one `set_stream_sampling` of 1, 4 and 16 rows between two frames (host time until its table writes have completed);
  (d) the scalar frame on THIS library against another build of it (`--parent-lib`: the parent commit's librstnet_hip.so) through
      `tools/ab.py LIB=`, in alternating child processes (`bench.py --workload e2e --lm-batch 32`).

Medians of `--rounds` (7) rounds; every round measures each leg once, in alternating order.  Next to both ratios stands the spread
max / min of the same-session (same-library) samples of this very run: a ratio inside it is not a difference this run can show.

    python tools/bench_slot_sampling.py --parent-lib /path/to/parent/librstnet_hip.so --out profiles/slot_sampling.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pipeline_restart import _child, _ms_per_frame  # noqa: E402


def _samples(v, digits=4):
    return {"median": round(statistics.median(v), digits), "samples": [round(x, digits) for x in v]}


def against_parent(args):
    """(d): this library and the parent's in alternating child processes, the scalar `e2e_b32` frame of bench.py (a line on stderr per
    child: fourteen model loads take minutes)."""
    if not args.parent_lib:
        return {"skipped": "no --parent-lib given"}
    legs = {"this": [], "parent": []}
    for r in range(args.rounds):
        for name in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            legs[name].append(_child(args, args.parent_lib if name == "parent" else None))
            print(f"round {r}: {name} {legs[name][-1]:.4f} ms per frame", file=sys.stderr, flush=True)
    med = {k: statistics.median(v) for k, v in legs.items()}
    spread = {k: max(v) / min(v) for k, v in legs.items()}
    ratio, box = med["this"] / med["parent"], max(spread.values())
    return {"this_ms_per_frame": _samples(legs["this"]), "parent_ms_per_frame": _samples(legs["parent"]),
            "this_over_parent": round(ratio, 4), "same_library_spread_max_over_min": {k: round(v, 4) for k, v in spread.items()},
            "ratio_inside_same_library_spread": bool(1.0 / box <= ratio <= box)}


def in_process(args):
    """(a), (b) and (c): both sessions stay open (each owns its states; the weights are shared) and take turns."""
    import torch
    from rstnet_amd import _lib, ops, synth
    from rstnet_amd.codec.mimi import MimiCodec
    from rstnet_amd.lm.model import LMGen, LMModel
    from rstnet_amd.pipeline import StreamingPipeline
    dev = torch.device("cuda:0")
    B = args.batch
    cfg = dict(synth.LM_MOSHI_7B if args.lm_config == "moshi7b" else synth.LM_TINY_16Q)
    # two models on the same weight tensors: a model's streaming state belongs to one live session
    sd = synth.lm_state_dict(cfg, seed=0, device=str(dev))
    models = [LMModel.from_state_dict(sd, cfg) for _ in range(2)]
    mimi_sd = synth.mimi_state_dict(0)
    mimis = [MimiCodec.from_state_dict(mimi_sd).to(dev) for _ in range(2)]
    sets = [n for n in (1, 4, 16) if n <= B]
    total = args.warmup + args.rounds * args.frames + args.rounds * 2 * len(sets) + 4
    pcm = synth.synth_audio(B, 1920 * total, seed=200).to(dev)
    torch.manual_seed(1234)
    legs = {"scalar": [], "per_row": []}
    set_ms = {n: [] for n in sets}
    with StreamingPipeline(mimis[0], LMGen(models[0]), B, per_stream=True) as scalar, \
            StreamingPipeline(mimis[1], LMGen(models[1], per_stream_sampling=True), B, per_stream=True) as per_row:
        pipes = {"scalar": scalar, "per_row": per_row}
        at = {"scalar": 0, "per_row": 0}
        for name, pipe in pipes.items():
            _ms_per_frame(pipe, pcm, 0, args.warmup)
            at[name] = args.warmup
        for r in range(args.rounds):
            for name in (("scalar", "per_row") if r % 2 == 0 else ("per_row", "scalar")):
                legs[name].append(_ms_per_frame(pipes[name], pcm, at[name], args.frames))
                at[name] += args.frames
            # (c): n rows get new settings and seeds between two frames; the frames around it keep the session going
            for n in sets:
                rows = [(r + i) % B for i in range(n)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                per_row.set_stream_sampling(rows, temp=0.7 + 0.01 * r, top_k=100 + r, seed=[1000 * r + b for b in rows])
                torch.cuda.synchronize()
                set_ms[n].append((time.perf_counter() - t0) * 1e3)
                _ms_per_frame(per_row, pcm, at["per_row"], 2)
                at["per_row"] += 2
        graph_kept = per_row._fused is not None and per_row._fused.calls == 1
        # (b): the frame's noise launch alone, on the session's own tables and buffer
        sp = per_row.lm_gen._streaming_state.sampling
        frames_dev = per_row.lm_gen._streaming_state.offset_dev
        noise_us = []
        for r in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(5):
                ops.noise_exp_rows(sp.seed, frames_dev, sp.noise.shape[1], out=sp.noise)
            e0.record()
            for _ in range(args.noise_launches):
                ops.noise_exp_rows(sp.seed, frames_dev, sp.noise.shape[1], out=sp.noise)
            e1.record()
            torch.cuda.synchronize()
            noise_us.append(e0.elapsed_time(e1) * 1e3 / args.noise_launches)
        noise_shape = [B, int(sp.noise.shape[1])]
    med = {k: statistics.median(v) for k, v in legs.items()}
    spread = {k: max(v) / min(v) for k, v in legs.items()}
    ratio, box = med["per_row"] / med["scalar"], max(spread.values())
    return {"build_id": _lib.build_id(), "streams": B, "lm_config": args.lm_config, "frames_per_sample": args.frames, "rounds": args.rounds,
            "scalar_sampling_ms_per_frame": _samples(legs["scalar"]), "per_row_sampling_ms_per_frame": _samples(legs["per_row"]),
            "per_row_over_scalar": round(ratio, 4), "same_session_spread_max_over_min": {k: round(v, 4) for k, v in spread.items()},
            "per_row_ratio_inside_same_session_spread": bool(1.0 / box <= ratio <= box),
            "noise_launch_us": dict(_samples(noise_us, 3), shape=noise_shape, launches_per_sample=args.noise_launches,
                                    note="back-to-back launches between two HIP events: launch-rate bound at this size"),
            "set_stream_sampling_ms": {str(n): _samples(v) for n, v in set_ms.items()},
            "frame_graph_never_recaptured": bool(graph_kept)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lm-config", choices=["moshi7b", "tiny"], default="moshi7b")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40, help="timed frames per sample")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--noise-launches", type=int, default=200, help="launches between the two events of one noise sample")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's librstnet_hip.so (leg d); without it (d) is skipped")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--skip-in-process", action="store_true")
    ap.add_argument("--out", default=None, help="write the result here as JSON (it is always printed as one line)")
    args = ap.parse_args()
    # (d) first: its children must have the GPU's memory to themselves
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
