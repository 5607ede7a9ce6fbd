"""Headline benchmark: MimiCodec encode -> RVQ -> decode, batch = 64 x 10 s synthetic 24 kHz audio per GPU
(BASELINE.json configs[1]); metric = 12.5 Hz code frames per second, whole job.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path (encode + decode) over one batch that is already resident in HBM.
Multi-GPU: utterances are independent, so each rank owns its own batch (weak scaling); the only collective is the
one-off RCCL broadcast of the weights from rank 0 (`python bench.py --gpus N` spawns the N ranks itself when it was not
started by torchrun).  Rank 0 prints ONE JSON line with the contract fields (`metric`, `value`, `unit`, `ms_per_step` = the
mean of exactly --steps timed steps after --warmup untimed ones, ...).  That is all a plain run does.
`--dump-outputs DIR` writes what the last timed step computed (codec: `codes`, `wav`; lm / gpt: the frame's tokens; e2e: the
generated pcm) as DIR/<name>.npy in float32; the inputs are seeded, so two builds given the same arguments can be compared.
`--full` adds everything else the line used to carry:
  * `roofline` (dominant kernel: the fp32-MFMA windowed GEMM, timed per launch with HIP events on the launch stream in an
    extra instrumented step) and `cpu_baseline` (the CPU oracle timed on this host on a bounded sample),
  * `timing`: median / p95 of >= 50 individually synchronised steps, next to the contract's K-step mean,
  * `code_exact_match_vs_cpu_oracle` / `wav_rel_err_vs_cpu_oracle`: two clips of the batch through the CPU oracle (the
    "RVQ code-index exact-match" half of the metric), and
  * on the single-GPU run the sub-objects `lm_b1` (BASELINE configs[2]: Moshi-7B-shaped LMGen.step, batch 1) and `e2e_b1`
    (the north-star target: Mimi encode -> LMGen.step -> Mimi decode per 80 ms frame, batch 1), each with its own
    `ms_per_step`, `timing`, `roofline` and `cpu_baseline` (skip with --no-sub); the multi-GPU line carries `e2e_b32` instead.
The other workloads (--workload lm / e2e / gpt) likewise time their steps only, and add `timing`, `roofline` and `cpu_baseline`
under --full.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("NO_TORCH_COMPILE", "1")

import torch  # noqa: E402

METRIC = "codec+LM audio frames/sec (24 kHz, 12.5 Hz tokens) at batch=1 and batch=64; RVQ code-index exact-match"   # BASELINE.json
FP32_MFMA_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2516.6  # same guide: v_mfma_f32_32x32x16_bf16, 32 cycles per SIMD -> 16 x the f32 instruction (dense)
# the large GEMMs run every fp32 product as SIX bf16 matrix-instruction products (three-plane split operands, gemm_win.hip): their
# roofline in algorithmic (fp32) flops is the bf16 peak / 6
B3_EQUIV_PEAK_TFLOPS = round(BF16_MFMA_PEAK_TFLOPS / 6, 1)
FRAME_HOP = 1920


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64, help="utterances per GPU")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--workload", choices=["codec", "lm", "e2e", "gpt"], default="codec",
                    help="codec = BASELINE configs[1] (the default, headline); lm = configs[2]: Moshi-7B-shaped RQ-Transformer decode, "
                         "batch 1; e2e = configs[3] shape per GPU; gpt = configs[4]: Qwen-0.5B-shaped litgpt backbone + LoRA, batch 32")
    ap.add_argument("--lm-config", choices=["moshi7b", "tiny"], default="moshi7b")
    ap.add_argument("--lm-batch", type=int, default=None, help="lm / e2e / gpt: concurrent streams per GPU (<= 64; default 1, gpt 32)")
    ap.add_argument("--greedy", action="store_true", help="lm: greedy decoding instead of temperature / top-k sampling")
    ap.add_argument("--fp8", action="store_true", help="gpt: fp8 (e4m3, per-row scales) matrix-core path for the global blocks")
    ap.add_argument("--lm-context", type=int, default=0, help="lm: start the timed frames at this ring offset (e.g. 3000 = every "
                    "temporal attention reads the full 3000-slot KV ring; the ring content is zeros, the bytes are the same)")
    ap.add_argument("--kv-dtype", choices=["bf16", "f32"], default="bf16", help="lm / e2e: precision of the temporal KV rings (bf16 = the "
                    "reference's cache precision, the default; f32 = the fp32 parity setting)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-dist", action="store_true", help="run the multi-GPU code path (RCCL process group, weight broadcast as one blob, "
                    "rank pinning, barriers, all-gather of per-rank times) even at --gpus 1: the only RCCL execution a 1-GPU box can give")
    ap.add_argument("--layers", action="store_true", help="print the per-launch GEMM table (shape, ms, TFLOP/s, GB/s) to stderr")
    ap.add_argument("--no-check", action="store_true", help="codec: skip the parity sample (2 clips through the CPU oracle: code "
                    "exact-match of encode, waveform error of decode)")
    ap.add_argument("--check", action="store_true", help=argparse.SUPPRESS)      # the parity sample is on by default since round 2
    ap.add_argument("--no-sub", action="store_true", help="codec: skip the lm_b1 / e2e_b1 sub-benchmarks of the single-GPU line")
    ap.add_argument("--sub-steps", type=int, default=60, help="timed frames of the lm_b1 / e2e_b1 sub-benchmarks (>= 50: median + p95)")
    ap.add_argument("--timing-samples", type=int, default=50, help="individually synchronised steps behind `timing` (median, p95)")
    ap.add_argument("--full", action="store_true", help="measure and check everything beyond the headline figure: `roofline` (extra "
                    "instrumented step), `timing` samples, the parity sample, the CPU baselines and, on the codec line, the sub-benchmarks "
                    "of the other configurations.  Without it a run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last timed step computed "
                    "as DIR/<name>.npy (float32; at most 64 MB in all, beyond that a fixed seeded sample of every array)")
    args = ap.parse_args()
    if args.lm_batch is None:
        args.lm_batch = 32 if args.workload == "gpt" else 1
    return args


def pmc_traffic(kernel: str, workload: str):
    """HBM bytes per launch of `kernel` from the committed PMC summary of this workload (tools/pmc_traffic.py over two
    rocprofv3 --pmc passes of this very command; FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md), or None.
    The counters cannot be read from inside the process, so the number is the profiled run's, not this run's."""
    import glob
    best = None
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", f"*_{workload}_pmc_traffic.json"))):
        try:
            with open(path) as f:
                tab = json.load(f)
        except (OSError, ValueError):
            continue
        rows = [v for name, v in tab.items() if isinstance(v, dict) and name.startswith(kernel)]
        n = sum(v["launches"] for v in rows)
        if n:      # all template instances of the kernel, launch-weighted (the latest summary wins)
            best = {"bytes_per_launch": round(sum(v["traffic_bytes_per_launch"] * v["launches"] for v in rows) / n),
                    "fetch_bytes_per_launch": round(sum(v["fetch_bytes_per_launch"] * v["launches"] for v in rows) / n),
                    "write_bytes_per_launch": round(sum(v["write_bytes_per_launch"] * v["launches"] for v in rows) / n),
                    "launches_profiled": n, "source": f"profiles/{os.path.basename(path)}"}
    return best


def _loaded_build_id():
    from rstnet_amd import _lib
    return _lib.build_id()


def rocprof_avg_ms(kernel: str, workload: str):
    """Average launch duration of `kernel` (all template instances whose name starts with it) in the committed
    `rocprofv3 --kernel-trace --stats` summary of this workload (profiles/*_{workload}_kernel_stats.csv, the latest), or None.
    The cross-check of the live HIP-event figure: event pairs around a 5 us launch add a few us of their own, the trace does not.
    `stale`: the summary was taken with ANOTHER build of the library than the one loaded now (its `.meta.json`, tools/profile_meta.py,
    names the build id; a summary without one is stale by definition) -- callers then do not quote it."""
    import csv
    import glob
    paths = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", f"*_{workload}_kernel_stats.csv")))
    if not paths:
        return None
    calls = total = 0.0
    with open(paths[-1], newline="") as f:
        for r in csv.DictReader(f):
            if r["kernel"].startswith(kernel):      # (str.startswith takes a tuple of prefixes as well)
                calls += float(r["calls"])
                total += float(r["total_us"])
    if not calls:
        return None
    built = None
    try:
        with open(paths[-1][:-4] + ".meta.json") as f:
            built = json.load(f).get("build_id")
    except (OSError, ValueError):
        pass
    loaded = _loaded_build_id()
    return {"avg_launch_ms": round(total / calls / 1e3, 5), "launches_profiled": int(calls), "source": f"profiles/{os.path.basename(paths[-1])}",
            "build_id": built, "loaded_build_id": loaded, "stale": built is None or built != loaded}


def mfma_counters(kernel: str, peak: float = FP32_MFMA_PEAK_TFLOPS):
    """Matrix-pipe busy fraction and sustained shader clock of `kernel` (all instances whose name starts with it, time-weighted) from
    the committed PMC summary profiles/*_codec_mfma.json (tools/pmc_mfma.py: SQ_VALU_MFMA_BUSY_CYCLES, GRBM_GUI_ACTIVE), or None.
    The chip clocks to its power budget: under these kernels it sustains ~2.2 GHz, not the 2.4 GHz the nominal peak is priced at."""
    import glob
    paths = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "*_codec_mfma.json")))
    if not paths:
        return None
    try:
        with open(paths[-1]) as f:
            tab = json.load(f)
    except (OSError, ValueError):
        return None
    rows = [v for name, v in tab.items() if isinstance(v, dict) and name.startswith(kernel)]
    ms = sum(v["total_ms"] for v in rows)
    if not ms:
        return None
    busy = sum(v["mfma_pipe_busy_frac"] * v["total_ms"] for v in rows) / ms
    clk = sum(v["shader_clock_ghz"] * v["total_ms"] for v in rows) / ms
    return {"busy_frac": round(busy, 4), "shader_clock_ghz": round(clk, 3),
            "peak_at_that_clock_tflops": round(peak * clk / 2.4, 1),
            "launches_profiled": int(sum(v["launches"] for v in rows)), "source": f"profiles/{os.path.basename(paths[-1])}"}


def _with_rocprof(roofline: dict, kernel: str, workload: str, per_launch: float, peak: float) -> dict:
    """Adds the trace-based figures next to the live ones: `per_launch` algorithmic bytes (GB/s) or flop (TFLOP/s) per launch."""
    r = rocprof_avg_ms(kernel, workload)
    if r is not None:
        ach = per_launch / (r["avg_launch_ms"] * 1e-3) / (1e9 if roofline["unit"] == "GB/s" else 1e12)
        r.update({"achieved": round(ach, 1 if roofline["unit"] == "GB/s" else 3), "frac": round(ach / peak, 4)})
    roofline["rocprof"] = r
    return roofline


def _settle_roofline(r: dict, ms_step: float) -> dict:
    """Which figure a decode line's `achieved` / `frac` quote.  The live figure of these lines comes from HIP event
    pairs around every launch of one EAGER frame; around 8-20 us launches the pairs add several us each, so for the batched lines
    their sum exceeds the graph-replayed frame and the fraction describes the instrumentation.  Rule: the kernel-trace figure of the
    SAME workload (`rocprof`: average launch duration in the committed `rocprofv3 --kernel-trace --stats` summary) is the headline
    whenever such a summary exists; the event-pair numbers move to `event_pairs` (flagged when they exceed the step); with neither a
    trace nor a sound event sum, the whole-frame figure (frame bytes / step time) is quoted."""
    live = {"achieved": r["achieved"], "frac": r["frac"], "avg_launch_ms": r.pop("avg_launch_ms", None),
            "kernel_ms_per_step": r.pop("kernel_ms_per_step", None), "share_of_step": r.pop("share_of_step_eager", None),
            "method": "HIP event pairs around every launch of one eager (ungraphed) frame"}
    inflated = (live["kernel_ms_per_step"] or 0.0) > ms_step
    if inflated:
        live["exceeds_step"] = True
        live["note"] = "the event pairs themselves add several us per launch: the sum exceeds the graph-replayed frame -- not evidence"
    rp = r.get("rocprof")
    if rp and rp.get("stale"):
        r["stale"] = True       # the committed trace belongs to another build: not quoted (ADVICE r5 / VERDICT r5 #4)
    if rp and rp.get("frac") is not None and not rp.get("stale"):
        r["achieved"], r["frac"] = rp["achieved"], rp["frac"]
        r["avg_launch_ms"] = rp["avg_launch_ms"]
        r["kernel_ms_per_step"] = round(rp["avg_launch_ms"] * r.get("launches_per_step", 0), 3)
        r["frac_source"] = f"kernel trace: {rp['source']}"
    elif (inflated or (rp and rp.get("stale"))) and r.get("frame"):
        r["achieved"], r["frac"] = r["frame"]["achieved"], r["frame"]["frac"]
        r["frac_source"] = ("whole frame: algorithmic bytes / step time (" + ("the committed kernel trace was taken with another build of the library"
                            if rp and rp.get("stale") else "no kernel trace of this workload under profiles/") + ")")
    else:
        r["avg_launch_ms"], r["kernel_ms_per_step"] = live["avg_launch_ms"], live["kernel_ms_per_step"]
        r["frac_source"] = "HIP event pairs (live)"
    r["event_pairs"] = live
    return r


def cpu_baseline(sd, seconds_per_clip: float, batch: int = 4):
    """The CPU restatement (oracle/mimi_oracle.py, validated bit-exact against the imported reference) on this host."""
    from oracle import mimi_oracle as O
    from rstnet_amd import synth
    cfg = O.MimiConfig()
    audio = synth.synth_audio(batch, int(seconds_per_clip * 24000), seed=11)
    default_threads = torch.get_num_threads()
    best, best_threads = None, default_threads
    with torch.no_grad():
        # torch's CPU convolutions stop scaling well before 128 threads: time the default and a 32-thread setting
        for threads in sorted({default_threads, min(32, default_threads)}):
            torch.set_num_threads(threads)
            for _ in range(2):
                t0 = time.perf_counter()
                codes = O.encode(sd, cfg, audio)
                O.decode(sd, cfg, codes)
                dt = time.perf_counter() - t0
                if best is None or dt < best:
                    best, best_threads = dt, threads
    # SURVEY 8(d) also asks for the single-thread figure: one 2 s clip, one thread
    torch.set_num_threads(1)
    one = synth.synth_audio(1, 2 * 24000, seed=11)
    with torch.no_grad():
        t0 = time.perf_counter()
        c1 = O.encode(sd, cfg, one)
        O.decode(sd, cfg, c1)
        dt1 = time.perf_counter() - t0
    torch.set_num_threads(default_threads)
    frames = codes.shape[0] * codes.shape[2]
    return {"value": round(frames / best, 2), "unit": "frames/s", "cores": best_threads, "kind": "port",
            "single_thread": {"value": round(c1.shape[0] * c1.shape[2] / dt1, 2), "unit": "frames/s", "cores": 1,
                              "sample": f"oracle encode+decode of one 2 s clip, 1 thread ({dt1:.2f} s)"},
            "sample": f"oracle encode+decode of {batch} x {seconds_per_clip:g} s clips, fp32, torch CPU, best of "
                      f"{{{min(32, default_threads)}, {default_threads}}} threads x 2 runs ({best:.2f} s); host has "
                      f"{os.cpu_count()} logical cores"}


HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)


# what a multi-GPU run reports next to the contract's line (rank 0 prints it under "multi_gpu"): per-rank step times, the weight
# broadcast (bytes, wall time), the host CPUs each rank was pinned to
MULTI: dict = {}
FORCE_DIST = False      # --force-dist: the process-group path of --gpus N (nccl init, weight broadcast, barriers, all-gather of the rank times) at N = 1


def _dist(world: int) -> bool:
    return world > 1 or FORCE_DIST


def _broadcast_stats(key: str):
    b = MULTI.get(key)
    return None if not b else {"bytes": int(b["bytes"]), "seconds": round(b["seconds"], 4),
                               "gb_per_s": round(b["bytes"] / max(b["seconds"], 1e-9) / 1e9, 2),
                               "note": "one flat blob per model, RCCL broadcast from rank 0; not in the timed region"}


def _multi_gpu_block(world: int):
    if not _dist(world):
        return None
    blk = {"per_rank_ms_per_step": MULTI.get("per_rank_ms_per_step"), "host": MULTI.get("host"),
           "weight_broadcast": _broadcast_stats("broadcast"),
           # the 15.4 GB LM blob (bf16) of the sharded end-to-end line: the one collective the multi-GPU design rests on
           "lm_weight_broadcast": _broadcast_stats("broadcast_lm"),
           "forced_at_world_1": bool(FORCE_DIST and world == 1),
           "scaling_note": "no scaling curve has been measured on hardware by the builder: the driver computes efficiency from its own per-N runs"}
    return blk


def _timing(samples_ms):
    """median / p95 of individually synchronised steps (median + p95 over >= 50 iterations)."""
    xs = sorted(samples_ms)
    p95 = xs[min(len(xs) - 1, int(round(0.95 * (len(xs) - 1))))]
    return {"median_ms": round(statistics.median(xs), 4), "p95_ms": round(p95, 4), "min_ms": round(xs[0], 4), "samples": len(xs),
            "method": "wall clock around each step, torch.cuda.synchronize() on both sides"}


def _sample_steps(step, n):
    out = []
    for i in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(i)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _quiesce_host():
    """Before a timed region: collect what earlier sub-benchmarks left behind NOW (captured graphs of a finished session are destroyed
    when the cycle collector finds them -- tens of milliseconds if that happens inside the next timed loop)."""
    import gc
    gc.collect()
    torch.cuda.synchronize()


DUMP_BUDGET_BYTES = 64_000_000


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: every tensor of `arrays` as out_dir/<name>.npy in float32 (code and token ids are < 2^24: exact).  A set larger
    than DUMP_BUDGET_BYTES keeps the same seeded sample of flat positions of each array on every run, so that two builds given the same
    arguments can be compared element for element.  `None` entries (no output yet in a streaming step) are skipped."""
    import numpy as np
    arrays = {k: v for k, v in arrays.items() if v is not None}
    keep = min(1.0, DUMP_BUDGET_BYTES / max(1, sum(4 * v.numel() for v in arrays.values())))
    os.makedirs(out_dir, exist_ok=True)
    for name, v in arrays.items():
        x = v.detach().cpu().float()
        if keep < 1.0:
            x = x.reshape(-1)
            idx = torch.randperm(x.numel(), generator=torch.Generator().manual_seed(0))[:int(x.numel() * keep)].sort().values
            x = x[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), x.numpy())


def _timed_loop(step, warmup, steps, world, dev):
    """The contract's timing: `warmup` untimed steps, then EXACTLY `steps` steps between barrier + synchronize on both sides,
    MAX over ranks.  `step(i)` runs step number i (0-based over warm-up + timed)."""
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    _quiesce_host()
    if _dist(world):
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(warmup + i)
    torch.cuda.synchronize()
    if _dist(world):
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if _dist(world):
        mine = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        MULTI["per_rank_ms_per_step"] = [round(float(t.item()) / steps * 1e3, 3) for t in every]
        elapsed = max(float(t.item()) for t in every)           # the contract's figure: the slowest rank
    return elapsed


def _host_mem_available_gb() -> float:
    try:
        with open("/proc/meminfo") as f:
            for ln in f:
                if ln.startswith("MemAvailable:"):
                    return int(ln.split()[1]) / 1e6
    except OSError:
        pass
    return 0.0


def _timing_only_state_dict(cfg: dict):
    """fp32 weights of the reference's key layout for TIMING the oracle at the real 7B shape: every tensor is cut from one tiled block of
    uniform numbers scaled like synth.lm_state_dict's init (drawing 7.7 B numbers from a seeded CPU generator would take minutes and a
    matrix-vector product's time does not depend on the values)."""
    from rstnet_amd import synth
    shapes = {k: (tuple(v.shape), float(v.float().abs().max())) for k, v in synth.lm_state_dict(dict(cfg, num_layers=1), 0).items()}
    block = torch.rand(1 << 24) * 2 - 1
    sd = {}

    def make(shape, scale):
        n = 1
        for d in shape:
            n *= d
        t = block.repeat(-(-n // block.numel()))[:n].view(*shape) if n > block.numel() else block[:n].clone().view(*shape)
        return t * scale if "alpha" not in key else 1.0 + 0.1 * t
    for l in range(cfg["num_layers"]):
        for key0, (shape, scale) in shapes.items():
            if key0.startswith("transformer.layers.0."):
                key = key0.replace("transformer.layers.0.", f"transformer.layers.{l}.")
                sd[key] = make(shape, scale)
    for key, (shape, scale) in shapes.items():
        if not key.startswith("transformer.layers."):
            sd[key] = make(shape, scale)
    return sd


def lm_cpu_baseline(frames: int = 2):
    """The LM oracle (oracle/lm_oracle.py = models/model.py:490-562 at the sizes of moshi/models/loaders.py:68-98) on this host, batch 1,
    greedy, fp32: the SAME workload as the GPU line -- 32 temporal layers x 4096 + the 8-step depth transformer -- for `frames` frames
    after one warm-up frame (VERDICT r5 missing #3; 31 GB of fp32 weights).  A host with less than 96 GB available times the round-5
    stand-in instead (a Qwen-0.5B-sized temporal stack) and says so."""
    from oracle import lm_oracle as L
    from rstnet_amd import synth
    full = _host_mem_available_gb() >= 96.0
    if full:
        cfg = dict(synth.LM_MOSHI_7B)
        sd = _timing_only_state_dict(cfg)
    else:
        frames = max(frames, 6)
        cfg = dict(synth.LM_MOSHI_7B, dim=1024, num_heads=16, num_layers=24, context=3000)
        sd = {k: v.float() for k, v in synth.lm_state_dict(cfg, 0).items()}
    gen = L.LMGenOracle(sd, L.LMConfig(**cfg), 1)
    user = torch.randint(0, cfg["card"], (frames + 1, 1, cfg["n_q"] - cfg["dep_q"], 1))
    with torch.no_grad():
        gen.step(user[0])
        t0 = time.perf_counter()
        for s in range(frames):
            gen.step(user[s + 1])
        dt = time.perf_counter() - t0
    shape = (f"temporal {cfg['num_layers']} x {cfg['dim']} (the 7B shape of the GPU line: {sum(v.numel() for v in sd.values()) / 1e9:.2f} B parameters, weights cut "
             f"from a tiled random block -- timing only)" if full else
             "temporal 24 x 1024 (Qwen-0.5B-sized STAND-IN: this host has < 96 GB available for the 31 GB of fp32 weights)")
    del gen, sd
    return {"value": round(frames / dt, 3), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port", "same_size_as_gpu_line": full,
            "sample": f"oracle LMGen greedy, {frames} frames after one warm-up frame, batch 1, fp32, {shape} + the real 8-step depth "
                      f"transformer (6 x 1024); {dt / frames:.2f} s per frame", "_seconds_per_frame": dt / frames}


def e2e_cpu_baseline(lm_cpu: dict, frames: int = 6):
    """End-to-end CPU leg = the LM oracle's frame time (above) + the codec oracle's encode and decode of the same number of
    80 ms frames of ONE stream (fp32, torch CPU)."""
    from oracle import mimi_oracle as O
    from rstnet_amd import synth
    sd, cfg = synth.mimi_state_dict(0), O.MimiConfig()
    audio = synth.synth_audio(1, frames * FRAME_HOP, seed=12)
    with torch.no_grad():
        O.decode(sd, cfg, O.encode(sd, cfg, audio))
        t0 = time.perf_counter()
        O.decode(sd, cfg, O.encode(sd, cfg, audio))
        codec_s = (time.perf_counter() - t0) / frames
    per_frame = codec_s + lm_cpu["_seconds_per_frame"]
    return {"value": round(1.0 / per_frame, 2), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"per frame: codec oracle encode + decode of {frames} frames of one stream ({codec_s * 1e3:.0f} ms / frame) + the LM "
                      f"oracle leg of lm_b1 ({lm_cpu['_seconds_per_frame'] * 1e3:.0f} ms / frame, "
                      f"{'the 7B shape' if lm_cpu.get('same_size_as_gpu_line') else 'Qwen-0.5B-sized stand-in'})"}


def build_lm(args, rank, world, dev, stats_key="broadcast"):
    from rstnet_amd import synth
    from rstnet_amd.lm.model import LMModel
    cfg = dict(synth.LM_MOSHI_7B if args.lm_config == "moshi7b" else synth.LM_TINY)
    # weights: generated on rank 0's device (bf16), then ONE RCCL broadcast over xGMI; the other ranks build their replica on
    # views of the received blob
    sd = synth.lm_state_dict(cfg, seed=0, device=str(dev)) if rank == 0 else None
    if _dist(world):
        from rstnet_amd.parallel import broadcast_state_dict
        sd = broadcast_state_dict(sd, dev, src=0, stats=MULTI.setdefault(stats_key, {}))
    n_params = sum(v.numel() for v in sd.values())
    return cfg, LMModel.from_state_dict(sd, cfg, kv_dtype=torch.bfloat16 if args.kv_dtype == "bf16" else torch.float32), n_params


def run_lm(args, rank, world, dev, lm=None, steps=None, warmup=None, cpu=True, dump=None):
    """BASELINE configs[2]: one step = one 80 ms frame of LMGen.step (temporal step + 8 depth steps + sampling).  Returns the
    result dict on rank 0 (None elsewhere).  `dump`: directory for the last timed frame's tokens (--dump-outputs)."""
    from rstnet_amd import ops
    from rstnet_amd.lm.model import LMGen
    cfg, model, n_params = lm if lm is not None else build_lm(args, rank, world, dev)
    B = args.lm_batch
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    n_samples = max(args.timing_samples, 1)
    gen = LMGen(model, use_sampling=not args.greedy, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    user = torch.randint(0, cfg["card"], (warmup + steps + n_samples + 1, B, cfg["n_q"] - cfg["dep_q"], 1), generator=g, device=dev)
    torch.manual_seed(1234 + rank)
    with gen.streaming(B):
        if args.lm_context:
            st = model.transformer._streaming_state
            st.pos.fill_(args.lm_context)
            st.offset_cpu = args.lm_context
        last = {}

        def step(i):
            last["tokens"] = gen.step(user[i])
        elapsed = _timed_loop(step, warmup, steps, world, dev)
        if dump and rank == 0:
            dump_outputs(dump, last)
        samples = _sample_steps(lambda i: gen.step(user[warmup + steps + i]), n_samples) if args.full else None
        # which form the timed frames' temporal stack took (ops.TEMPORAL_FRAME = "auto": the persistent launch from 2048 ring steps on)
        temporal_path = ("one persistent launch (rst_temporal_decode_frame)" if getattr(model.transformer._streaming_state, "tables", None) is not None
                         else "five launches per layer")
    if rank != 0:
        return None
    ms_frame = elapsed / steps * 1e3
    result = {
        "metric": METRIC,
        "value": round(B * world * steps / elapsed, 2), "unit": "frames/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": round(ms_frame, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "bf16 weights, f32 activations", "data": "synthetic",
        "config": {"workload": f"LMGen.step (temporal + 8-step depth transformer + sampling), BASELINE.json configs[2], {args.lm_config}",
                   "batch_per_gpu": B, "params": n_params, "context_frames": args.lm_context + warmup + steps,
                   "kv_dtype": str(model.kv_dtype).replace("torch.", "") if hasattr(model, "kv_dtype") else "float32",
                   "sampling": "greedy" if args.greedy else "temp 0.8/0.7 top-k 250/25", "hip_graphs": True,
                   "temporal_stack": temporal_path, "parallelism": f"replica x{world}"},
        "x_realtime_per_stream": round(steps / elapsed / 12.5, 2),
    }
    if _dist(world):
        result["multi_gpu"] = _multi_gpu_block(world)
    if not args.full:
        return result
    # roofline of the dominant kernel (weight-streaming GEMV): one extra frame, eager (no graph), HIP events per launch
    os.environ["NO_CUDA_GRAPH"] = "1"
    gen2 = LMGen(model, use_sampling=not args.greedy)
    recs = []
    with gen2.streaming(B):
        gen2.step(user[0])
        ops.PROFILE = recs
        gen2.step(user[1])
        torch.cuda.synchronize()
        ops.PROFILE = None
    os.environ["NO_CUDA_GRAPH"] = "0"
    gemv = [r for r in recs if r[0] in ("gemv_bf16", "gemm_skinny")]
    ms = sum(r[1].elapsed_time(r[2]) for r in gemv)
    nbytes = sum(r[4] for r in gemv)
    # the depth phase at batch <= 2 is ONE persistent launch (rst_depth_decode_frame): its weight bytes count towards the frame
    depth = [r for r in recs if r[0] == "depth_frame"]
    depth_ms = sum(r[1].elapsed_time(r[2]) for r in depth)
    depth_bytes = sum(r[4] for r in depth)
    if args.layers:
        agg = {}
        for _, e0, e1, fl, nb, shp in gemv:
            d = agg.setdefault(shp, [0, 0.0, 0])
            d[0] += 1; d[1] += e0.elapsed_time(e1); d[2] += nb
        for shp, (n, t, nb) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"  gemv B,N,K={shp}: {n:4d} launches {t:8.3f} ms  {nb / t / 1e6:8.1f} GB/s", file=sys.stderr)
    timing = _timing(samples)
    frame_bytes = nbytes + depth_bytes
    kern = "gemv_" if B <= 2 else "gemm_skinny"       # packed and fp32-input (x32) forms of the bf16 skinny GEMM
    # the committed trace / counter summaries this line quotes: profiles/rNN_lm_* (batch 1), rNN_lm_ctx3000_*, rNN_lm32_* (tools/collect_profiles.sh)
    tag = "lm" if B <= 2 else f"lm{B}"
    if args.lm_context:
        tag += f"_ctx{args.lm_context}"
    result.update({
        "timing": timing,
        "roofline": {"bound": "hbm", "kernel": ("gemv_kernel / gemv_norm_kernel / gemv_ksplit_kernel" if B <= 2 else "gemm_skinny_kernel / gemm_skinny_x32_kernel") + " (bf16 weight streaming)",
                     "achieved": round(nbytes / ms / 1e6, 1),
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4),
                     "traffic": pmc_traffic(kern, tag) or (pmc_traffic(kern, "lm") if B <= 2 else None),
                     "algorithmic_bytes_per_launch": round(nbytes / max(1, len(gemv))), "launches_per_step": len(gemv), "avg_launch_ms": round(ms / max(1, len(gemv)), 5),
                     "kernel_ms_per_step": round(ms, 3), "algorithmic_gb_per_step": round(nbytes / 1e9, 3),
                     "share_of_step_eager": round(ms / ms_frame, 3),
                     # the whole frame against the HBM roofline: every algorithmic byte of the frame / the median frame time
                     "frame": {"algorithmic_gb": round(frame_bytes / 1e9, 3), "achieved": round(frame_bytes / timing["median_ms"] / 1e6, 1),
                               "frac": round(frame_bytes / timing["median_ms"] / 1e6 / HBM_PEAK_GBS, 4)},
                     "depth_frame": ({"kernel": "depth_frame_kernel (persistent: 8 steps x 6 layers + heads + samplers in one launch)",
                                      "ms": round(depth_ms, 4), "algorithmic_gb": round(depth_bytes / 1e9, 3),
                                      "achieved": round(depth_bytes / depth_ms / 1e6, 1), "frac": round(depth_bytes / depth_ms / 1e6 / HBM_PEAK_GBS, 4),
                                      "bound": "in-launch hand-off latency (~250 dependent all-to-all edges), not bandwidth"}
                                     if depth else None)},
    })
    _with_rocprof(result["roofline"], kern, tag, nbytes / max(1, len(gemv)), HBM_PEAK_GBS)
    if result["roofline"]["rocprof"] is None and B <= 2 and args.lm_context:
        # (same kernels, same bytes: only the attention launches differ at a full ring -- the batch-1 trace stands in, and says so)
        _with_rocprof(result["roofline"], kern, "lm", nbytes / max(1, len(gemv)), HBM_PEAK_GBS)
    _settle_roofline(result["roofline"], ms_frame)
    if cpu and not args.no_cpu_baseline and not _dist(world):    # the CPU leg is timed on rank 0 of the single-GPU run only
        result["cpu_baseline"] = lm_cpu_baseline()
    return result


def gpt_cpu_baseline(cfg_d, frames: int = 3):
    """oracle/gpt_oracle.py on this host at the benchmark's shape, ONE stream, greedy: streamed forward_global step + the
    dep_q codecformer steps per frame."""
    from oracle import gpt_oracle as Gp
    from rstnet_amd import synth
    keep = set(Gp.GPTConfig.__dataclass_fields__)
    cfg = Gp.GPTConfig(**{k: v for k, v in cfg_d.items() if k in keep})
    sd = {k: v.float() for k, v in synth.gpt_state_dict(cfg_d, 0, lora=False).items()}
    st = Gp.new_global_state(cfg, 1)
    tok = torch.randint(0, 2048, (1, cfg.num_codebooks, 1))
    with torch.no_grad():
        def frame():
            h, lg = Gp.forward_global(sd, cfg, tok, st, merged=True)
            cst = Gp.new_codecformer_state(cfg, 1)
            prev = lg.argmax(-1).view(1, 1, 1)
            for k in range(cfg.dep_q):
                prev = Gp.forward_codecformer(sd, cfg, k, prev, h, cst).argmax(-1).view(1, 1, 1)
        frame()
        t0 = time.perf_counter()
        for _ in range(frames):
            frame()
        dt = time.perf_counter() - t0
    return {"value": round(frames / dt, 2), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle GPT streamed step + {cfg.dep_q} codecformer steps, {frames} frames, batch 1 (the GPU line is batch "
                      f"32), greedy, fp32, LoRA pre-merged"}


def build_gpt(args, dev):
    from rstnet_amd import synth
    from rstnet_amd.lm.gpt import GPT, Config
    cfg_d = dict(synth.GPT_QWEN_0_5B if args.lm_config != "tiny" else synth.GPT_TINY_GQA)
    sd = synth.gpt_state_dict(cfg_d, seed=0, device=str(dev))
    model = GPT.from_state_dict(sd, Config.from_dict(cfg_d))
    del sd
    return cfg_d, model, sum(v.numel() for v in model.state_dict().values())


def run_gpt(args, rank, world, dev, gpt=None, fp8=None, steps=None, warmup=None, cpu=True, dump=None):
    """BASELINE configs[4]: Qwen-0.5B-shaped litgpt backbone (LoRA adapters merged at load) + codecformer, B streams; one step =
    one frame: text sample + dep_q depth steps with sampling (one graph) + the global T = 1 step of the completed frame (one
    graph).  Returns the result dict on rank 0 (None elsewhere).  `dump`: directory for the last timed frame's tokens (--dump-outputs)."""
    from rstnet_amd import ops
    from rstnet_amd.lm.generate import GPTGen
    cfg_d, model, n_params = gpt if gpt is not None else build_gpt(args, dev)
    fp8 = args.fp8 if fp8 is None else fp8
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    model.use_fp8(fp8)
    B = args.lm_batch
    n_codes = cfg_d["audio_card"] - 2
    gen = GPTGen(model, use_sampling=not args.greedy, temp=0.8, temp_text=0.7, top_k=250, top_k_text=25, n_audio_codes=n_codes)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    K = cfg_d["n_q"] + 1
    prompt = torch.randint(0, n_codes, (B, K, 8), generator=g, device=dev)
    torch.manual_seed(1234 + rank)
    gen.begin(B)
    gen.set_blanking([False] + [True] * (cfg_d["dep_q"] - 1))
    h, logits = gen.prefill(prompt)

    # first frame after the prompt, then every step = ONE graph replay: global step of the completed frame + text sample + dep_q
    # depth steps with their samples, on the session's device-resident token column (GPTGen.step)
    gen.start(h, logits)
    last = {}

    def frame(h, logits):
        last["text"], last["audio"] = gen.step()
        return h, logits
    for _ in range(warmup):
        h, logits = frame(h, logits)
    torch.cuda.synchronize()
    _quiesce_host()
    if _dist(world):
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        h, logits = frame(h, logits)
    torch.cuda.synchronize()
    if _dist(world):
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dump and rank == 0:
        dump_outputs(dump, last)
    samples = []
    for _ in range(max(args.timing_samples, 1) if args.full and not _dist(world) else 0):      # median / p95 of individually synchronised frames
        torch.cuda.synchronize()
        ts = time.perf_counter()
        h, logits = frame(h, logits)
        torch.cuda.synchronize()
        samples.append((time.perf_counter() - ts) * 1e3)
    gen.end()
    if _dist(world):
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank != 0:
        return None
    ms_frame = elapsed / steps * 1e3
    result = {
        "metric": METRIC,
        "value": round(B * world * steps / elapsed, 2), "unit": "frames/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": round(ms_frame, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": ("fp8 e4m3 block GEMMs, " if fp8 else "") + "bf16 weights, f32 activations (bf16 hi+lo split on the matrix cores)",
        "data": "synthetic",
        "config": {"workload": "GPT (Qwen-1.5-0.5B-shaped litgpt backbone, LoRA r=32 merged) + codecformer: streamed frame = global "
                               "step + text sample + 8 depth steps with sampling, BASELINE.json configs[4]",
                   "batch_per_gpu": B, "params": n_params, "sampling": "greedy" if args.greedy else "temp 0.8/0.7 top-k 250/25",
                   "hip_graphs": True,
                   "gemm_precision": "fp8 e4m3 (per-row scales) in the global blocks, bf16 hi+lo elsewhere" if fp8 else "bf16 hi+lo",
                   "parallelism": f"replica x{world}"},
        "x_realtime_per_stream": round(steps / elapsed / 12.5, 2),
    }
    if not args.full:
        return result
    # roofline of the weight-streaming GEMMs: one extra eager frame with HIP events per launch
    gen2 = GPTGen(model, use_sampling=not args.greedy, n_audio_codes=n_codes, noise=None)
    os.environ["NO_CUDA_GRAPH"] = "1"
    gen2.begin(B)
    h, logits = gen2.prefill(prompt)
    gen2.start(h, logits)
    gen2.step()
    recs = []
    ops.PROFILE = recs
    gen2.step()
    torch.cuda.synchronize()
    ops.PROFILE = None
    gen2.end()
    os.environ["NO_CUDA_GRAPH"] = "0"
    gemm = [r for r in recs if r[0] in ("gemv_bf16", "gemm_skinny", "gemm_skinny_fp8")]
    ms = sum(r[1].elapsed_time(r[2]) for r in gemm)
    nbytes = sum(r[4] for r in gemm)
    if args.layers:
        agg = {}
        for _, e0, e1, fl, nb, shp in gemm:
            d = agg.setdefault(shp, [0, 0.0, 0])
            d[0] += 1; d[1] += e0.elapsed_time(e1); d[2] += nb
        for shp, (n, t, nb) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"  gemm B,N,K={shp}: {n:4d} launches {t:8.3f} ms  {nb / t / 1e6:8.1f} GB/s", file=sys.stderr)
    # every weight byte a frame streams once: global blocks + LM head (bf16, or e4m3 + scales for the fp8 blocks), the stacked
    # codecformer_in, dep_q x (depth layers + head)
    c = cfg_d
    blk = c["n_layer"] * ((c["n_embd"] + 2 * c["n_query_groups"] * (c["n_embd"] // c["n_head"])) * c["n_embd"] + c["n_embd"] * c["n_embd"]
                          + 3 * c["intermediate_size"] * c["n_embd"])
    dE, dH = c["codecformer_dim"], (21 * c["codecformer_dim"]) // 8 if c["codecformer_dim_feedforward"] == 4 * c["codecformer_dim"] \
        else (2 * c["codecformer_dim_feedforward"]) // 3
    dep = c["dep_q"] * (c["codecformer_layers"] * (4 * dE * dE + 3 * dH * dE) + c["audio_card"] * dE + dE * c["n_embd"])
    frame_bytes = blk * (1 if fp8 else 2) + 2 * (c["padded_vocab_size"] * c["n_embd"] + dep)
    result["roofline"] = {"bound": "hbm", "kernel": ("gemv_kernel / gemv_norm_kernel / gemv_ksplit_kernel" if B <= 2 else "gemm_skinny_kernel / gemm_skinny_x32_kernel"
                                                     + (" / gemm_skinny_fp8_kernel" if fp8 else "")) + " (weight streaming)",
                          "achieved": round(nbytes / ms / 1e6, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                          "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4),
                          "traffic": pmc_traffic("gemv_" if B <= 2 else "gemm_skinny", "gpt"),
                          "algorithmic_bytes_per_launch": round(nbytes / max(1, len(gemm))), "launches_per_step": len(gemm),
                          "avg_launch_ms": round(ms / max(1, len(gemm)), 5), "kernel_ms_per_step": round(ms, 3),
                          "algorithmic_gb_per_step": round(nbytes / 1e9, 3), "share_of_step_eager": round(ms / ms_frame, 3),
                          # the whole frame against the HBM roofline: every weight byte of the frame once / the frame time
                          "frame": {"algorithmic_gb": round(frame_bytes / 1e9, 3), "achieved": round(frame_bytes / ms_frame / 1e6, 1),
                                    "frac": round(frame_bytes / ms_frame / 1e6 / HBM_PEAK_GBS, 4)}}
    if samples:
        result["timing"] = _timing(samples)
    tag = ("gpt_fp8" if fp8 else "gpt") if B > 2 else f"gpt{B}"
    result["roofline"]["traffic"] = pmc_traffic("gemv_" if B <= 2 else "gemm_skinny", tag)
    _with_rocprof(result["roofline"], "gemv_" if B <= 2 else "gemm_skinny", tag, nbytes / max(1, len(gemm)), HBM_PEAK_GBS)
    _settle_roofline(result["roofline"], ms_frame)
    if cpu and not args.no_cpu_baseline and not _dist(world):    # the CPU leg is timed on rank 0 of the single-GPU run only
        result["cpu_baseline"] = gpt_cpu_baseline(cfg_d)
    return result


def run_e2e(args, rank, world, dev, lm=None, steps=None, warmup=None, lm_result=None, stats_key="broadcast", dump=None):
    """BASELINE configs[3] shape on one GPU: B concurrent streams, each frame = Mimi encode (1920 samples) -> LMGen.step ->
    Mimi decode; value = B * frames / time.  Returns the result dict on rank 0.  `dump`: directory for the last timed frame's
    generated pcm (--dump-outputs)."""
    from rstnet_amd import synth
    from rstnet_amd.codec.mimi import MimiCodec
    from rstnet_amd.lm.model import LMGen
    from rstnet_amd.pipeline import StreamingPipeline
    cfg, model, n_params = lm if lm is not None else build_lm(args, rank, world, dev)
    B = args.lm_batch
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    n_samples = max(args.timing_samples, 1)
    mimi_sd = synth.mimi_state_dict(0) if rank == 0 else None
    if _dist(world):
        from rstnet_amd.parallel import broadcast_state_dict
        mimi_sd = broadcast_state_dict(mimi_sd, dev, src=0, stats=MULTI.setdefault(stats_key, {}))
    mimi = MimiCodec.from_state_dict(mimi_sd).to(dev)
    gen = LMGen(model, use_sampling=not args.greedy)
    pcm = synth.synth_audio(B, 1920 * (warmup + steps + n_samples), seed=200 + rank).to(dev)
    torch.manual_seed(1234 + rank)
    last = {}
    with StreamingPipeline(mimi, gen, B) as pipe:
        step = lambda s: pipe.step(pcm[:, :, s * 1920:(s + 1) * 1920].contiguous())     # noqa: E731
        elapsed = _timed_loop(lambda s: last.update(pcm=step(s)), warmup, steps, world, dev)
        if dump and rank == 0:
            dump_outputs(dump, last)
        samples = _sample_steps(lambda i: step(warmup + steps + i), n_samples) if args.full else None
    if rank != 0:
        return None
    codec_bytes = 4 * sum(v.numel() for k, v in mimi_sd.items() if v.is_floating_point())
    lm_bytes = lm_result["roofline"]["frame"]["algorithmic_gb"] * 1e9 if lm_result else None
    result = {
        "metric": METRIC,
        "value": round(B * world * steps / elapsed, 2), "unit": "frames/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": round(elapsed / steps * 1e3, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "codec f32; LM bf16 weights, f32 activations", "data": "synthetic",
        "config": {"workload": f"end-to-end streaming: Mimi encode -> LMGen.step -> Mimi decode, BASELINE.json configs[3] shape, {args.lm_config}",
                   "streams_per_gpu": B, "parallelism": f"replica x{world}, streams sharded"},
        "x_realtime_per_stream": round(steps / elapsed / 12.5, 2)}
    if args.full:
        timing = result["timing"] = _timing(samples)
    if _dist(world):
        result["multi_gpu"] = _multi_gpu_block(world)
    if args.full and lm_bytes is not None:
        # the frame is weight streaming end to end -- every LM weight byte once (bf16) and every codec weight once (fp32: encoder +
        # decoder halves, each streamed once per frame whatever the number of streams)
        total = lm_bytes + codec_bytes
        lr = lm_result["roofline"]
        # (the LM's launches only: the codec's own fp32 `gemv_kernel<.., true, ..>` launches are not part of the byte count above)
        kern = ("gemv_norm_kernel", "gemv_ksplit_kernel") if B <= 2 else ("gemm_skinny_kernel", "gemm_skinny_x32_kernel")
        tag = f"e2e{B}"
        frame = {"algorithmic_gb": round(total / 1e9, 3), "lm_gb": round(lm_bytes / 1e9, 3), "codec_weight_gb": round(codec_bytes / 1e9, 3),
                 "achieved": round(total / timing["median_ms"] / 1e6, 1), "frac": round(total / timing["median_ms"] / 1e6 / HBM_PEAK_GBS, 4)}
        # dominant kernel of the frame = the LM's weight-streaming launches (same launches, same bytes as the lm line), timed by the
        # kernel trace of THIS workload (profiles/rNN_e2e{B}_kernel_stats.csv); without one the whole-frame figure is quoted
        r = {"bound": "hbm", "kernel": lr["kernel"] + " inside the end-to-end frame", "unit": "GB/s", "peak": HBM_PEAK_GBS,
             "achieved": frame["achieved"], "frac": frame["frac"], "traffic": pmc_traffic(kern, tag) or lr.get("traffic"),
             "algorithmic_bytes_per_launch": lr["algorithmic_bytes_per_launch"], "launches_per_step": lr["launches_per_step"],
             "algorithmic_gb_per_step": frame["algorithmic_gb"], "frame": frame,
             "frac_source": "whole frame: algorithmic bytes (LM frame + codec weights) / median step time"}
        rp = rocprof_avg_ms(kern, tag)
        if rp is not None:
            ach = lr["algorithmic_bytes_per_launch"] / (rp["avg_launch_ms"] * 1e-3) / 1e9
            rp.update({"achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBS, 4)})
            if rp.get("stale"):
                r["stale"] = True       # another build's trace: the whole-frame figure above stays the headline
            else:
                r.update(achieved=rp["achieved"], frac=rp["frac"], avg_launch_ms=rp["avg_launch_ms"],
                         kernel_ms_per_step=round(rp["avg_launch_ms"] * lr["launches_per_step"], 3), frac_source=f"kernel trace: {rp['source']}")
        r["rocprof"] = rp
        result["roofline"] = r
    return result


def _free_port() -> int:
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def spawn_command(n_gpus: int, argv, port: int):
    """The launch line of the contract: one rank per GPU of one node, rendezvous on 127.0.0.1."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def parity_sample(model, sd_cpu, audio, codes, n=2, timed_wav=None):
    """The "RVQ code-index exact-match" half of the metric on the first `n` clips of the timed batch: encode against the CPU
    oracle's codes, decode (of the oracle's codes, as its own small batch) against the oracle's waveform -- and `timed_wav`, the
    waveform the TIMED step decoded at the full batch (the decode plan the benchmark measures), against the oracle's for every
    sampled clip whose codes equal the oracle's."""
    from oracle import mimi_oracle as O
    n = min(n, audio.shape[0])
    cfg = O.MimiConfig()
    with torch.no_grad():
        ref_codes = O.encode(sd_cpu, cfg, audio[:n].cpu())
        ref_wav = O.decode(sd_cpu, cfg, ref_codes)
        wav = model.decode(ref_codes.to(audio.device)).cpu()
    got = codes[:n].cpu()
    match = float((got == ref_codes).float().mean())
    err = float((wav - ref_wav).abs().max() / ref_wav.abs().max())
    timed_err = None
    if timed_wav is not None:
        same = [i for i in range(n) if torch.equal(got[i], ref_codes[i])]
        if same:
            tw = timed_wav[:n].cpu()[same]
            timed_err = float(f"{float((tw - ref_wav[same]).abs().max() / ref_wav[same].abs().max()):.3e}")
    return round(match, 6), float(f"{err:.3e}"), n, timed_err


def make_summary(head: dict, subs: dict) -> dict:
    """One compact object with every BASELINE configuration of the line: `<name>_ms` (per step / frame), `<name>_xrt` (x real time per
    stream), `<name>_frac` (the roofline fraction of that sub-object's dominant kernel).  Short keys, scalars only -- it must fit the
    tail of the line the driver keeps."""
    def rf(d):
        r = d.get("roofline") or {}
        return r.get("frac")
    s = {"codec_b64_ms": head["ms_per_step"], "codec_b64_frames_s": head["value"], "codec_b64_frac": rf(head),
         "codec_b64_code_match": head.get("code_exact_match_vs_cpu_oracle"), "codec_b64_wav_err": head.get("timed_batch_wav_rel_err_vs_cpu_oracle")}
    for name, d in subs.items():
        s[f"{name}_ms"] = d.get("ms_per_step")
        s[f"{name}_xrt"] = d.get("x_realtime_per_stream")
        s[f"{name}_frac"] = rf(d)
    return s


def main():
    args = parse()
    global FORCE_DIST
    FORCE_DIST = bool(args.force_dist)
    if FORCE_DIST and args.gpus == 1 and "WORLD_SIZE" not in os.environ:
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", LOCAL_WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # not started by torchrun: spawn the ranks ourselves (same command line) and relay their output
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        sys.exit(subprocess.call(spawn_command(args.gpus, sys.argv[1:], _free_port()), env=env))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback)"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if _dist(world):
        import torch.distributed as dist
        from rstnet_amd.parallel import pin_rank_threads
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # eight ranks replaying graphs and launching ~100 kernels per step from one host: disjoint, NUMA-near CPU slices per rank
        MULTI["host"] = pin_rank_threads(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
        dist.init_process_group("nccl", device_id=dev)

    if args.workload in ("lm", "e2e", "gpt"):
        if args.workload == "gpt":
            res = run_gpt(args, rank, world, dev, dump=args.dump_outputs)
            if rank == 0:
                print(json.dumps(res), flush=True)
        else:
            lm = build_lm(args, rank, world, dev)
            if args.workload == "lm":
                res = run_lm(args, rank, world, dev, lm=lm, dump=args.dump_outputs)
            else:
                # the frame's byte count and dominant-kernel launches come from a short LM-only pass (as on the default line)
                lm_res = run_lm(args, rank, world, dev, lm=lm, steps=4, warmup=3, cpu=False) if args.full else None
                res = run_e2e(args, rank, world, dev, lm=lm, lm_result=lm_res, dump=args.dump_outputs)
            if rank == 0:
                res.get("cpu_baseline", {}).pop("_seconds_per_frame", None)
                print(json.dumps(res), flush=True)
        if _dist(world):
            dist.barrier()
            dist.destroy_process_group()
        return

    from rstnet_amd import ops, synth
    from rstnet_amd.codec.mimi import MimiCodec
    from rstnet_amd.parallel import broadcast_state_dict

    # weights: generated on rank 0 only, then ONE RCCL broadcast over xGMI
    sd_cpu = synth.mimi_state_dict(0) if rank == 0 else None
    if _dist(world):
        sd_dev = broadcast_state_dict(sd_cpu, dev, src=0, template=lambda: synth.mimi_state_dict(0), stats=MULTI.setdefault("broadcast", {}))
        model = MimiCodec.from_state_dict({k: v for k, v in sd_dev.items()}).to(dev)
    else:
        model = MimiCodec.from_state_dict(sd_cpu).to(dev)

    T = int(args.seconds * 24000)
    audio = synth.synth_audio(args.batch, T, seed=100 + rank).to(dev)   # rank-private utterances, resident in HBM
    frames_per_step = args.batch * (-(-T // FRAME_HOP))
    last = {}

    def step(_i=0):
        codes = model.encode(audio)
        last["codes"], last["wav"] = codes, model.decode(codes)

    elapsed = _timed_loop(step, args.warmup, args.steps, world, dev)
    codes, timed_wav = last["codes"], last["wav"]
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"codes": codes, "wav": timed_wav})

    # ---- roofline of the dominant kernel: one extra instrumented step, HIP events around every GEMM launch
    roofline = None
    if rank == 0 and args.full:
        ops.PROFILE = []
        step()
        torch.cuda.synchronize()
        recs, ops.PROFILE = ops.PROFILE, None
        if args.layers:
            for i, (_, e0, e1, fl, nb, shp) in enumerate(recs):
                ms = e0.elapsed_time(e1)
                print(f"  gemm[{i:3d}] M={shp[0]:9d} N={shp[1]:5d} K={shp[2]:5d}  {ms:8.3f} ms  {fl / ms / 1e9:7.2f} TFLOP/s  "
                      f"{nb / ms / 1e6:8.1f} GB/s(min traffic)", file=sys.stderr)
        t_step_ms = elapsed / args.steps * 1e3
        per_kernel = {}
        for name, e0, e1, fl, nb, shp in recs:
            d = per_kernel.setdefault(name, {"ms": 0.0, "flops": 0.0, "launches": 0})
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["launches"] += 1
        dom = max(per_kernel, key=lambda k: per_kernel[k]["ms"])     # the dominant kernel of the step
        d = per_kernel[dom]
        tf = d["flops"] / (d["ms"] * 1e-3) / 1e12
        all_flops = sum(v["flops"] for v in per_kernel.values())
        b3 = dom == "gemm_win_b3"
        prefix = f"{dom}_stream" if b3 else f"{dom}_"       # (not the one-off weight-packing launches of the same family)
        peak = B3_EQUIV_PEAK_TFLOPS if b3 else FP32_MFMA_PEAK_TFLOPS
        label = (f"{dom}_stream_kernel (v_mfma_f32_32x32x16_bf16: operands split into three bf16 planes, six products per fp32 product, f32 accumulate)"
                 if b3 else f"{dom}_*kernel (fp32 v_mfma_f32_32x32x2_f32)")

        def peak_of(name):
            return B3_EQUIV_PEAK_TFLOPS if name in ("gemm_win_b3", "resblock_b3") else FP32_MFMA_PEAK_TFLOPS
        roofline = {"bound": "mfma", "kernel": label, "achieved": round(tf, 3),
                    "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4),
                    "traffic": pmc_traffic(prefix, "codec"), "mfma_pipe": mfma_counters(prefix, peak), "launches_per_step": d["launches"],
                    "avg_launch_ms": round(d["ms"] / d["launches"], 4),
                    "kernel_ms_per_step": round(d["ms"], 3), "share_of_step": round(d["ms"] / t_step_ms, 3),
                    "algorithmic_gflop_per_step": round(d["flops"] / 1e9, 1),
                    "other_kernels": {k: {"ms_per_step": round(v["ms"], 3), "launches": v["launches"],
                                          "achieved_tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2),
                                          "frac": round(v["flops"] / (v["ms"] * 1e-3) / 1e12 / peak_of(k), 4)}
                                      for k, v in per_kernel.items() if k != dom},
                    # the whole step: every algorithmic flop of the GEMM-shaped launches / the step time, against the f32 instruction's peak
                    # (the figure the step would be capped at without the bf16 split)
                    "step": {"algorithmic_gflop": round(all_flops / 1e9, 1), "achieved": round(all_flops / t_step_ms / 1e9, 3),
                             "frac_of_f32_mfma_peak": round(all_flops / t_step_ms / 1e9 / FP32_MFMA_PEAK_TFLOPS, 4)}}
        if b3:
            roofline["peak_note"] = (f"algorithmic (fp32) flops against the bf16 dense peak {BF16_MFMA_PEAK_TFLOPS} / 6 products; "
                                     f"the f32 matrix instruction's peak is {FP32_MFMA_PEAK_TFLOPS}")
            roofline["x_f32_mfma_peak"] = round(tf / FP32_MFMA_PEAK_TFLOPS, 3)
        _with_rocprof(roofline, prefix, "codec", d["flops"] / d["launches"], peak)

    result = None
    if rank == 0:
        total_frames = frames_per_step * world * args.steps
        result = {
            "metric": METRIC,
            "value": round(total_frames / elapsed, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (large GEMMs: operands as three bf16 planes, six bf16 matrix-instruction products per fp32 product, f32 accumulate)",
            "data": "synthetic",
            "config": {"workload": "MimiCodec encode->RVQ(8x2048x256)->decode, BASELINE.json configs[1]",
                       "batch_per_gpu": args.batch, "clip_seconds": args.seconds, "sample_rate": 24000,
                       "frames_per_step_per_gpu": frames_per_step, "weights": "random-init (rstnet_amd.synth seed 0)",
                       "parallelism": f"replica x{world}, utterances sharded, RCCL weight broadcast only"},
            "x_realtime_per_stream": round(total_frames / elapsed / 12.5 / (args.batch * world), 1),
        }
        if args.full:
            result["roofline"] = roofline
        if _dist(world):
            result["multi_gpu"] = _multi_gpu_block(world)
        if args.full and not _dist(world):
            result["timing"] = _timing(_sample_steps(step, max(args.timing_samples, 1)))
        if args.full and not args.no_check:
            match, err, n, timed_err = parity_sample(model, sd_cpu, audio, codes, timed_wav=timed_wav)
            result["code_exact_match_vs_cpu_oracle"] = match
            result["wav_rel_err_vs_cpu_oracle"] = err
            result["timed_batch_wav_rel_err_vs_cpu_oracle"] = timed_err
            result["parity_sample"] = (f"{n} clips x {args.seconds:g} s of the timed batch: encode codes vs oracle/mimi_oracle.py, decode of the oracle's "
                                       f"codes vs its waveform, and the waveform the timed step decoded at batch {args.batch} vs the oracle's")
        if args.full and not args.no_cpu_baseline and not _dist(world):    # the CPU leg is timed on rank 0 of the single-GPU run only
            result["cpu_baseline"] = cpu_baseline(sd_cpu, args.seconds)
    if args.full and _dist(world) and not args.no_sub:
        # BASELINE configs[3] on the multi-GPU line: end-to-end streaming with 32 streams PER GPU (256 over 8 GPUs),
        # streams sharded over the ranks, the LM's weights (15.4 GB of bf16) generated on rank 0 and handed to the others by ONE RCCL
        # broadcast -- what MLLM_v2/moshi/models/loaders.py:142-159 does per process from disk and
        # egs/pretraining/local/offline_codec_tokenization.py:45-51 does per rank.  No data-path collective: the timed frames touch
        # the ranks' own streams only; value = all ranks' frames / the slowest rank's time.
        del audio, last, codes, timed_wav
        model = None
        torch.cuda.empty_cache()
        args.lm_batch = 32
        lm = build_lm(args, rank, world, dev, stats_key="broadcast_lm")
        e2e = run_e2e(args, rank, world, dev, lm=lm, steps=args.sub_steps, warmup=10, stats_key="broadcast_e2e_codec")
        del lm
        if rank == 0:
            for k in ("metric", "higher_is_better", "scaling", "vs_baseline", "data"):
                e2e.pop(k, None)
            result["e2e_b32"] = e2e
            lb = e2e["multi_gpu"].get("lm_weight_broadcast") or {}
            result["summary"] = {"codec_b64_ms": result["ms_per_step"], "codec_b64_frames_s": result["value"],
                                 "codec_per_rank_ms": (result.get("multi_gpu") or {}).get("per_rank_ms_per_step"),
                                 "e2e_b32_ms": e2e["ms_per_step"], "e2e_b32_frames_s": e2e["value"], "e2e_b32_xrt": e2e["x_realtime_per_stream"],
                                 "e2e_streams_total": 32 * world, "e2e_per_rank_ms": e2e["multi_gpu"].get("per_rank_ms_per_step"),
                                 "lm_broadcast_gb": round(lb.get("bytes", 0) / 1e9, 2), "lm_broadcast_gb_s": lb.get("gb_per_s"),
                                 "codec_broadcast_gb_s": ((result.get("multi_gpu") or {}).get("weight_broadcast") or {}).get("gb_per_s")}
    if args.full and not _dist(world) and not args.no_sub:
        # the north-star targets ride on the same line: batch-1 LM decode and the batch-1 end-to-end streaming frame
        del audio, last, codes, timed_wav
        model = None
        torch.cuda.empty_cache()
        args.lm_batch = 1
        lm = build_lm(args, rank, world, dev)
        lm_res = run_lm(args, rank, world, dev, lm=lm, steps=args.sub_steps, warmup=10)
        e2e_res = run_e2e(args, rank, world, dev, lm=lm, steps=args.sub_steps, warmup=10, lm_result=lm_res)
        if not args.no_cpu_baseline and "cpu_baseline" in lm_res:
            e2e_res["cpu_baseline"] = e2e_cpu_baseline(lm_res["cpu_baseline"])
            lm_res["cpu_baseline"].pop("_seconds_per_frame", None)
        subs = {"lm_b1": lm_res, "e2e_b1": e2e_res}
        lm_cpu, e2e_cpu = lm_res.get("cpu_baseline"), e2e_res.get("cpu_baseline")

        def shared_cpu(leg, of):
            return dict(leg, note=f"the CPU leg of {of} (one stream; not re-timed for this sub-object)") if leg else None
        # configs[2] with every temporal attention reading a full 3000-slot ring; configs[3] at its per-GPU size (32 streams)
        args.lm_context = 3000
        subs["lm_ctx3000"] = run_lm(args, rank, world, dev, lm=lm, steps=args.sub_steps, warmup=10, cpu=False)
        args.lm_context, args.lm_batch = 0, 32
        subs["lm_b32"] = run_lm(args, rank, world, dev, lm=lm, steps=args.sub_steps, warmup=10, cpu=False)
        subs["e2e_b32"] = run_e2e(args, rank, world, dev, lm=lm, steps=args.sub_steps, warmup=10, lm_result=subs["lm_b32"])
        for name, leg, of in (("lm_ctx3000", lm_cpu, "lm_b1"), ("lm_b32", lm_cpu, "lm_b1"), ("e2e_b32", e2e_cpu, "e2e_b1")):
            if leg:
                subs[name]["cpu_baseline"] = shared_cpu(leg, of)
        del lm
        torch.cuda.empty_cache()
        # configs[4]: Qwen-0.5B-shaped GPT + LoRA, 32 streams, bf16 hi+lo and the fp8 block GEMMs
        gpt = build_gpt(args, dev)
        subs["gpt_b32"] = run_gpt(args, rank, world, dev, gpt=gpt, fp8=False, steps=args.sub_steps, warmup=10)
        subs["gpt_b32_fp8"] = run_gpt(args, rank, world, dev, gpt=gpt, fp8=True, steps=args.sub_steps, warmup=10, cpu=False)
        if "cpu_baseline" in subs["gpt_b32"]:
            subs["gpt_b32_fp8"]["cpu_baseline"] = shared_cpu(subs["gpt_b32"]["cpu_baseline"], "gpt_b32")
        for sub in subs.values():      # sub-objects: drop what the enclosing line already states
            for k in ("metric", "n_gpus", "higher_is_better", "scaling", "vs_baseline", "data"):
                sub.pop(k, None)
        result.update(subs)
        # LAST key of the line (the driver keeps a 2 000-character tail): every configuration's time, rate and roofline fraction
        result["summary"] = make_summary(result, subs)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if _dist(world):
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
