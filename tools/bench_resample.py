"""A/B of the device-side sample-rate conversion against the host route, both legs in ONE process, interleaved.

(a) offline: ``MimiTokenizer.tokenize_batch`` of 64 x 10 s at 16 kHz int16 and at 44.1 kHz fp32, host route (torch-CPU resample file by
    file, padded fp32 batch at 24 kHz uploaded) against ``resample="device"`` (padded raw batch uploaded, one launch): wall time of the
    whole call, upload and the final ``.cpu()`` included; and the resample launch alone (device events).
(b) live: ``StreamingPipeline.step`` at B = 1 and B = 32 on the tiny LM, ``client_rate=48000`` against ``None``: ms per frame.

Every leg is warmed up, repeated, and reported as median / min / max; a leg counts as faster only outside the +-3 % box-to-box
spread README.md states.  Needs a GPU (no fallback).  Writes one JSON file (default ``profiles/resample_ab.json``).

    python tools/bench_resample.py [--reps 7] [--out profiles/resample_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DEV = "cuda:0"


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def verdict(host, dev):
    r = dev["median_ms"] / host["median_ms"]
    return {"device_over_host": round(r, 4), "verdict": "device faster" if r < 0.97 else ("host faster" if r > 1.03 else "inside the +-3 % spread")}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def bench_offline(reps, utterances, seconds):
    from rstnet_amd import synth
    from rstnet_amd.codec import audio_resample as AR
    from rstnet_amd.codec.mimi import MimiCodec
    from rstnet_amd.codec.tokenizer import MimiTokenizer
    tok = MimiTokenizer(MimiCodec.from_state_dict(synth.mimi_state_dict(0)).to(DEV))
    out = {}
    for rate, dtype in ((16000, torch.int16), (44100, torch.float32)):
        g = torch.Generator().manual_seed(rate)
        T = int(seconds * rate)
        wavs = [0.1 * torch.randn(T - 37 * i, generator=g) for i in range(utterances)]
        if dtype == torch.int16:
            wavs = [(w * 32768).round().clamp(-32768, 32767).to(torch.int16) for w in wavs]

        def host():        # what a caller with files of this type does today: to fp32 on the host, then the host route
            return tok.tokenize_batch([w.float() / 32768.0 if w.dtype == torch.int16 else w for w in wavs], rate)

        def device():
            return tok.tokenize_batch(wavs, rate, resample="device")

        a, b = host(), device()            # warm-up of both routes (every shape of the timed window), and what they agree on
        agree = sum(float((x == y).float().mean()) for x, y in zip(a, b)) / len(a)
        host(), device()
        t_host, t_dev = [], []
        for _ in range(reps):
            t_host.append(wall(host))
            t_dev.append(wall(device))
        # the resample launch alone, on the batch the device route uploads
        batch = torch.zeros(utterances, T, dtype=dtype)
        for r, w in enumerate(wavs):
            batch[r, :w.numel()] = w
        xb, lens = batch.to(DEV), torch.tensor([w.numel() for w in wavs], dtype=torch.int32, device=DEV)
        for _ in range(3):
            AR.resample_device(xb, lens, rate, 24000)
        ev = []
        for _ in range(max(reps, 10)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            AR.resample_device(xb, lens, rate, 24000)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        # the host resample alone, as the host route runs it (file by file)
        t_cpu = []
        for _ in range(3):
            t0 = time.perf_counter()
            for w in wavs:
                AR.resample(w.float() / 32768.0 if w.dtype == torch.int16 else w, rate, 24000)
            t_cpu.append(1e3 * (time.perf_counter() - t0))
        h, d = stats(t_host), stats(t_dev)
        out[f"{rate}_{'s16' if dtype == torch.int16 else 'f32'}"] = {
            "utterances": utterances, "seconds_each": seconds, "tokenize_batch_host": h, "tokenize_batch_device": d, **verdict(h, d),
            "resample_launch_alone": stats(ev), "host_resample_alone": stats(t_cpu), "torch_threads": torch.get_num_threads(),
            "upload_bytes_host_route": 4 * utterances * (-(-24000 * T // rate)), "upload_bytes_device_route": batch.element_size() * batch.numel(),
            "code_agreement_host_vs_device": round(agree, 6)}
    return out


def bench_live(reps, frames):
    from rstnet_amd import synth
    from rstnet_amd.codec.loaders import get_mimi
    from rstnet_amd.lm.model import LMGen, LMModel
    from rstnet_amd.pipeline import StreamingPipeline
    cfg = dict(synth.LM_TINY_16Q)
    mimi_sd = synth.mimi_state_dict(0)
    lm_sd = {k: v.to(DEV) for k, v in synth.lm_state_dict(cfg, seed=9).items()}
    out = {}
    for B in (1, 32):
        pipes = {}
        for name, rate in (("codec_rate", None), ("client_48k", 48000)):
            gen = LMGen(LMModel.from_state_dict(lm_sd, cfg), use_sampling=False)
            pipes[name] = StreamingPipeline(get_mimi(mimi_sd, device=DEV), gen, B, client_rate=rate).__enter__()
        try:
            g = torch.Generator().manual_seed(B)
            pcm = {k: (0.1 * torch.randn(B, 1, p.client_frame, generator=g)).to(DEV) for k, p in pipes.items()}
            for k, p in pipes.items():               # past the delay line and the capture of the fused frame
                for _ in range(p.lm_gen.max_delay + 6):
                    p.step(pcm[k])
            t = {k: [] for k in pipes}
            for _ in range(reps):
                for k, p in pipes.items():           # alternating blocks of `frames` frames
                    t[k].append(wall(lambda: [p.step(pcm[k]) for _ in range(frames)]) / frames)
            h, d = stats(t["codec_rate"]), stats(t["client_48k"])
            out[f"B{B}"] = {"frames_per_block": frames, "ms_per_frame_client_rate_none": h, "ms_per_frame_client_rate_48000": d,
                            "added_ms_per_frame": round(d["median_ms"] - h["median_ms"], 4)}
        finally:
            for p in pipes.values():
                p.__exit__(None, None, None)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_ab.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample needs a GPU: nothing is measured without one")
    from rstnet_amd import _lib
    res = {"tool": "tools/bench_resample.py", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "offline": bench_offline(args.reps, args.utterances, args.seconds), "live": bench_live(args.reps, args.frames)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
