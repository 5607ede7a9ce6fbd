"""Batched generation of ragged prompts against the same prompts one by one, and the uniform batch-32 frame of this library against
another build's: one run, legs interleaved.

    python tools/bench_gpt_ragged.py [--repeats 7] [--prompts 32] [--frames 24] [--lm-config qwen0.5b|tiny] [--parent-lib PATH]
                                     [--out profiles/gpt_ragged_batch.json]

Workload: ``--prompts`` utterances in the reference's TTS layout at the Qwen-0.5B shape (synthetic weights, as ``bench.py --workload
gpt``), text prefixes spread evenly over 40 .. 200 positions, ``--frames`` frames to generate each, greedy decoding, captured graphs.
Legs (a, b) in ONE process, interleaved, ``--repeats`` rounds after one untimed round, wall clock around each leg with a device
synchronisation on both sides:
  (a) batch     ``InferenceImp.generate_batch`` over all prompts: one ragged prefill on a per-stream session, lock-step frames
  (b) serial    ``InferenceImp.generate`` prompt by prompt: what the library offered before per-stream positions
Reported: utterance-frames/s of each (median over the rounds) and their ratio; how many prompts gave identical tokens in both.
Leg (c), with ``--parent-lib``: the uniform scalar-position ``gpt_b32`` session -- ``bench.py --workload gpt`` through ``tools/ab.py``,
one child process per sample, this tree's library and ``LIB=<parent>`` alternating, ``--repeats`` samples each.  Scalar-position launches
pass through kernels whose parameter blocks grew by the per-stream fields; the leg says whether that shows.  Reported: ms per frame of
each sample, the medians, their ratio, and the spread (max / min) of the same-library samples of this run -- a ratio inside that spread
is no measured difference.  Build the other library from its commit into a scratch directory (``git archive <commit> rstnet_amd/csrc
include | tar -x -C <dir> && make -C <dir>/rstnet_amd/csrc``) and pass ``<dir>/rstnet_amd/librstnet_hip.so``.
Writes the JSON line to ``--out`` and prints it."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from rstnet_amd import _lib, synth  # noqa: E402
from rstnet_amd.lm.generate import GenIds, InferenceImp  # noqa: E402
from rstnet_amd.lm.gpt import GPT, Config  # noqa: E402


def tts_prompts(cfg_d, ids: GenIds, n: int, frames: int, lo: int, hi: int):
    """``n`` utterances ``[K, L_i]``: ``n_text_i`` text ids then ``text_empty`` on row 0, audio ids below, two trailing padding columns;
    the prefix is the ``n_text_i`` text positions (spread evenly over ``lo .. hi``), ``frames`` frames remain to be generated."""
    g = torch.Generator().manual_seed(4321)
    K, n_pad = cfg_d["n_q"] + 1, 2
    text_hi = min(ids.text_empty_token, ids.text_pad_token, cfg_d["padded_vocab_size"])
    out = []
    for i in range(n):
        n_text = lo + (hi - lo) * i // max(1, n - 1)
        L = n_text + frames + n_pad
        seq = torch.randint(0, ids.n_audio_codes, (K, L), generator=g)
        seq[0, :n_text] = torch.randint(0, text_hi, (n_text,), generator=g)
        seq[0, n_text:] = ids.text_empty_token
        seq[1:, L - n_pad:] = ids.semantic_pad_token
        out.append(seq)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def uniform_sample(lib, lm_config: str, steps: int) -> float:
    """ms per frame of one ``bench.py --workload gpt`` child (batch 32, graph-replayed frames) on ``lib`` (None: this tree's)."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "ab.py")] + ([f"LIB={lib}"] if lib else []) + \
          ["--", "--workload", "gpt", "--steps", str(steps), "--warmup", "10", "--no-cpu-baseline"] + (["--lm-config", "tiny"] if lm_config == "tiny" else [])
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed:\n{res.stderr[-2000:]}")
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--uniform-steps", type=int, default=200)
    ap.add_argument("--lm-config", choices=["qwen0.5b", "tiny"], default="qwen0.5b")
    ap.add_argument("--parent-lib", default=None, help="another build of librstnet_hip.so for the uniform leg (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt_ragged_batch.json"))
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats: at least 7 (the figures are medians over the rounds)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tiny = a.lm_config == "tiny"
    cfg_d = dict(synth.GPT_TINY_GQA if tiny else synth.GPT_QWEN_0_5B)
    ids = GenIds(text_pad_token=319, text_empty_token=318, semantic_pad_token=31, n_audio_codes=30, text_initial_token_id=7) if tiny else GenIds()
    lo, hi = (4, 20) if tiny else (40, 200)
    seqs = tts_prompts(cfg_d, ids, a.prompts, a.frames, lo, hi)
    model = GPT.from_state_dict(synth.gpt_state_dict(cfg_d, seed=0, device=str(dev)), Config.from_dict(cfg_d))
    imp = InferenceImp(None, model, "sample", 0.7, 25, 0.8, 250, "TTS", use_sampling=False, ids=ids)
    legs = {"batch": lambda: imp.generate_batch(seqs), "serial": lambda: [imp.generate(s) for s in seqs]}
    outs = {k: fn() for k, fn in legs.items()}                      # one untimed round: packed weights, scratch, graph pools
    frames = {k: sum(o["frames"].shape[0] for o in v) for k, v in outs.items()}
    same = sum(torch.equal(x["frames"], y["frames"]) and torch.equal(x["text"], y["text"]) for x, y in zip(outs["batch"], outs["serial"]))
    rounds = []
    for _ in range(a.repeats):
        r = {}
        for k, fn in legs.items():
            bench._quiesce_host()
            r[k] = round(timed(fn)[0], 5)
        rounds.append(r)
        print(f"round {len(rounds)}: {r}", file=sys.stderr, flush=True)
    med = {k: statistics.median(r[k] for r in rounds) for k in legs}
    fps = {k: round(frames[k] / med[k], 2) for k in legs}
    out = {"tool": "tools/bench_gpt_ragged.py", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(dev), "lm_config": a.lm_config,
           "prompts": a.prompts, "prefix_lengths": [lo + (hi - lo) * i // max(1, a.prompts - 1) for i in range(a.prompts)],
           "frames_per_prompt": a.frames, "decoding": "greedy, captured graphs", "repeats": a.repeats,
           "method": "wall clock around each leg (device synchronised on both sides), legs interleaved (batch, serial) in one process after "
                     "one untimed round; medians over the rounds; a leg includes opening its sessions, the prefill and the per-frame host reads",
           "utterance_frames": frames, "prompts_with_identical_tokens": f"{same}/{a.prompts}",
           "median_s": {k: round(v, 5) for k, v in med.items()}, "rounds_s": rounds,
           "utterance_frames_per_s": fps, "batch_over_serial": round(fps["batch"] / fps["serial"], 3), "uniform_gpt_b32": None}
    del model, imp, legs, outs
    bench._quiesce_host()
    torch.cuda.empty_cache()
    if a.parent_lib:
        samples = {"this": [], "parent": []}
        for _ in range(a.repeats):
            samples["this"].append(uniform_sample(None, a.lm_config, a.uniform_steps))
            samples["parent"].append(uniform_sample(os.path.abspath(a.parent_lib), a.lm_config, a.uniform_steps))
            print(f"uniform gpt_b32 ms per frame: this {samples['this'][-1]} parent {samples['parent'][-1]}", file=sys.stderr, flush=True)
        m = {k: statistics.median(v) for k, v in samples.items()}
        out["uniform_gpt_b32"] = {
            "method": f"bench.py --workload gpt --steps {a.uniform_steps} --warmup 10 through tools/ab.py, one child process per sample, this tree's "
                      "library and LIB=<parent> alternating; ms per frame of the scalar-position batch-32 session",
            "ms_per_frame": samples, "median_ms": {k: round(v, 4) for k, v in m.items()},
            "this_over_parent": round(m["this"] / m["parent"], 4),
            "same_library_spread": {k: round(max(v) / min(v), 4) for k, v in samples.items()}}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
