"""What serving N conversations over one frame graph costs on the host side, at the `e2e_b32` shape (32 rows, Moshi-7B-shaped synthetic
LM, sampling on; one process, the legs measured in turns, medians of `--rounds` (7) rounds):

  (a) wall time per tick of `StreamingPipeline.step_packed` WITH the staging fill (`slots.pack_staged`) and the record parse
      (`slots.parse_records`), against the same pipeline's `step` surrounded by what a per-row server loop does with the older surface:
      per row a numpy conversion of the payload and a small upload, then `.cpu()` per valid row, `PcmFramer.encode`, and `.item()` per
      text token.  Half of the rows speak f32, half s16.  Both legs run the same frame graph body; the difference is host traffic.
  (b) the two new launches alone (HIP events around 200 back-to-back launches each), next to the bytes they move;
  (c) after (a) has finished: host time of the join part of a tick -- ONE `reset_streams(rows)` plus the rows' format words, until the writes have completed --
      for 1, 4 and 16 rows at once (one row alone: `reset_one_row_ms` of profiles/pipeline_per_stream.json).

    python tools/bench_slot_server.py --out profiles/slot_server.json
"""
import argparse
import json
import os
import statistics
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stat(v, nd=4):
    return {"median": round(statistics.median(v), nd), "samples": [round(x, nd) for x in v]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lm-config", choices=["moshi7b", "tiny"], default="moshi7b")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=30, help="timed ticks per sample")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the result here as JSON (it is always printed as one line)")
    args = ap.parse_args()

    import torch
    from rstnet_amd import _lib, ops, synth
    from rstnet_amd import slots as SL
    from rstnet_amd.codec.mimi import MimiCodec
    from rstnet_amd.lm.model import LMGen, LMModel
    from rstnet_amd.pipeline import StreamingPipeline
    from rstnet_amd.server import PcmFramer
    dev = torch.device("cuda:0")
    B, F = args.batch, 1920
    cfg = dict(synth.LM_MOSHI_7B if args.lm_config == "moshi7b" else synth.LM_TINY_16Q)
    sd = synth.lm_state_dict(cfg, seed=0, device=str(dev))
    models = [LMModel.from_state_dict(sd, cfg) for _ in range(2)]       # the same weight tensors; a model's streaming state is one session's
    mimi_sd = synth.mimi_state_dict(0)
    mimis = [MimiCodec.from_state_dict(mimi_sd).to(dev) for _ in range(2)]
    fmt = [SL.FMT_F32 if b % 2 == 0 else SL.FMT_S16 for b in range(B)]
    framers = [PcmFramer(F, SL.FMT_NAMES[f]) for f in fmt]
    n_frames = 8                                                       # the clients' audio repeats with this period
    audio = synth.synth_audio(B, F * n_frames, seed=200).numpy()
    payload = [[framers[b].encode(audio[b, 0, i * F:(i + 1) * F]) for b in range(B)] for i in range(n_frames)]
    torch.manual_seed(1234)
    legs = {"packed": [], "per_row": []}
    joins = {1: [], 4: [], 16: []}
    joins = {k: v for k, v in joins.items() if k <= B}

    with StreamingPipeline(mimis[0], LMGen(models[0]), B, per_stream=True) as packed, \
            StreamingPipeline(mimis[1], LMGen(models[1]), B, per_stream=True) as per_row:
        for b in range(B):
            packed.set_row_format(b, fmt[b])
        staged = packed.new_staged()
        staged_np = staged.numpy()
        pcm_dev = torch.zeros(B, 1, F, device=dev)
        sink = [0]

        def one_frame(framer, raw):
            framer.append_bytes(raw)
            return framer.frames()[0]

        def tick_packed(i):
            SL.pack_staged(staged_np, payload[i % n_frames], fmt, F)
            rec = SL.parse_records(packed.step_packed(staged).numpy(), F)
            sink[0] += sum(len(r[1]) for r in rec if r is not None)

        def tick_per_row(i):
            for b in range(B):                                          # what N handlers do today: convert on the host, upload the row
                pcm_dev[b, 0] = torch.from_numpy(one_frame(framers[b], payload[i % n_frames][b])).to(dev)
            wav = per_row.step(pcm_dev)
            if wav is None:
                return
            for b in per_row.stream_valid:
                out = framers[b].encode(wav[b, 0].cpu().numpy())
                sink[0] += len(out) + int(per_row.last_tokens[b, 0].item())

        def sample(fn, first):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(first, first + args.frames):
                fn(i)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.frames * 1e3

        ticks = {"packed": tick_packed, "per_row": tick_per_row}
        at = 0
        for name, fn in ticks.items():
            for i in range(args.warmup):
                fn(i)
        at = args.warmup
        assert packed._fused is not None and packed._fused.graph is not None and per_row._fused is not None
        for r in range(args.rounds):
            for name in (("packed", "per_row") if r % 2 == 0 else ("per_row", "packed")):
                legs[name].append(sample(ticks[name], at))
            at += args.frames
        # (c) after (a), not between its rounds: a reset row's rings start to fill again, which would shorten the packed leg's frames only.
        # The join part of a tick for k rows at once, then two frames so that the session goes on
        for r in range(args.rounds):
            for k in joins:
                rows = [(r * 5 + j * (B // k)) % B for j in range(k)]
                rows = sorted(set(rows))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                packed.reset_streams(rows)
                for b in rows:
                    packed.set_row_format(b, fmt[b])
                torch.cuda.synchronize()
                joins[k].append((time.perf_counter() - t0) * 1e3)
                tick_packed(at)
                tick_packed(at + 1)
        graph_kept = packed._fused.calls == 1

        # (b): the two launches alone
        REC = SL.record_stride(F)
        fmt_dev = torch.tensor(fmt, dtype=torch.int32, device=dev)
        st_dev = staged.to(dev)
        pcm = torch.zeros(B, 1, F, device=dev)
        wav = torch.from_numpy(audio[:, :, :F].copy()).to(dev)
        tokens = torch.zeros(B, cfg["dep_q"] + 1, dtype=torch.long, device=dev)
        off = torch.full((B,), 100, dtype=torch.long, device=dev)
        rec_dev = torch.zeros(B, REC, dtype=torch.uint8, device=dev)
        launches = {"frame_ingress": lambda: ops.frame_ingress(st_dev, fmt_dev, pcm),
                    "frame_egress": lambda: ops.frame_egress(wav, tokens, off, 1, fmt_dev, rec_dev)}
        kernel_us = {k: [] for k in launches}
        reps = 200
        for _ in range(args.rounds):
            for name, fn in launches.items():
                for _ in range(10):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                kernel_us[name].append(e0.elapsed_time(e1) / reps * 1e3)

    med = {k: statistics.median(v) for k, v in legs.items()}
    ratio = med["packed"] / med["per_row"]
    n_s16 = sum(1 for f in fmt if f == SL.FMT_S16)
    result = {
        "shape": "e2e_b32" if B == 32 and args.lm_config == "moshi7b" else f"e2e_b{B}_{args.lm_config}",
        "build_id": _lib.build_id(), "streams": B, "lm_config": args.lm_config, "sampling": True, "frames_per_sample": args.frames,
        "rounds": args.rounds, "formats": {"f32_rows": B - n_s16, "s16_rows": n_s16},
        "tick_ms": {"step_packed_with_fill_and_parse": _stat(legs["packed"]), "step_with_per_row_host_loop": _stat(legs["per_row"]),
                    "packed_over_per_row": round(ratio, 4), "faster_by_more_than_3_percent": bool(ratio < 0.97)},
        "launches_us": {k: _stat(v, 3) for k, v in kernel_us.items()},
        "launch_bytes": {"frame_ingress": {"read": 16 * B + sum(2 * F if f == SL.FMT_S16 else 4 * F for f in fmt) + 4 * B, "written": 4 * B * F},
                         "frame_egress": {"read": 4 * B * F + 8 * B + 8 * B + 4 * B, "written": B * REC},
                         "record_stride": REC, "per_tick_upload": B * REC, "per_tick_download": B * REC},
        "join_ms": {str(k): _stat(v) for k, v in joins.items()},
        "frame_graph_never_recaptured": bool(graph_kept),
        "note": "one machine, one run: figures move by about +-3 % from box to box; launches_us is back-to-back launch time under HIP events "
                "(launch overhead included: the kernels are shorter than a launch)",
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
