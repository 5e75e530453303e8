"""A frame of batch_stream.step_batched over B synthetic stream drivers, with their FeatureManagers in the slots of one FmHandle
(StreamDriver(features=...)) and in the drivers' own dicts, and the SfM input of 64 windows read in one call
against one call per window.

  leg slots  features=(handle, slot): one export, one set-depth, one second export, one slide and one add call per frame for all B
  leg dicts  the tracks / depth dicts and B Python loops

Both legs run in this process on the same streams, one after the other, and --repeats runs the measurement again that many times
with the order of the legs alternating.  A frame's time is the wall time of step_batched (the batched solve and marginalisation
included: the legs share them); reported per leg and B is the median over the frames after the first, with the least and the most.
Then tracks_batch over 64 slots against 64 tracks_get calls on the same tables (median of --reps).

    python tools/bench_stream_fm.py [--batches 1,64] [--frames 17] [--repeats 2] [--reps 20] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


STREAMS = {}


def run_leg(vio, hip, fh, B, n_frames, with_slots):
    bs, vs = vio.batch_stream, vio.stream
    drivers, sh = [], None
    for k in range(B):
        kw = dict(ctx_kwargs=dict(stream=sh)) if sh is not None else {}
        if with_slots:
            kw["features"] = (fh, k)
        if (k, n_frames) not in STREAMS:                  # (a driver only reads its stream: both legs and every repeat share it)
            STREAMS[(k, n_frames)] = vs.SyntheticStream(n_frames=n_frames, seed=k)
        drivers.append(vs.StreamDriver(hip, STREAMS[(k, n_frames)], triangulate=True, nonkey_every=4, **kw))
        sh = drivers[0].ctx.get_stream()
    marg = vio.load_marg().create(stream=sh)
    bs._check(drivers)
    times, active = [], list(drivers)
    while active:
        t0 = time.perf_counter()
        more = bs.step_batched(active, marg)
        times.append(1e3 * (time.perf_counter() - t0))
        active = [d for d, m in zip(active, more) if m]
    return times[1:], np.array([d.trajectory[-1][1][0:3] for d in drivers])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--frames", type=int, default=17)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vio = g.load_package()
    hip = vio.load_hip()
    fh = vio.load_fm().create()
    rows = []
    for rep in range(args.repeats):
        for B in [int(b) for b in args.batches.split(",")]:
            last = {}
            for leg in (("slots", "dicts") if rep % 2 == 0 else ("dicts", "slots")):
                wall, last[leg] = run_leg(vio, hip, fh, B, args.frames, leg == "slots")
                row = dict(repeat=rep, batch=B, leg=leg, frame_ms=float(np.median(wall)), frame_ms_min=float(np.min(wall)),
                           frame_ms_max=float(np.max(wall)), us_per_stream=1e3 * float(np.median(wall)) / B, frames=len(wall))
                rows.append(row)
                print("repeat %d  B %3d  leg %-5s  frame %9.3f ms (%.3f .. %.3f)  %9.1f us/stream" %
                      (rep, B, leg, row["frame_ms"], row["frame_ms_min"], row["frame_ms_max"], row["us_per_stream"]), flush=True)
            diff = float(np.abs(last["slots"] - last["dicts"]).max())
            rows.append(dict(repeat=rep, batch=B, last_position_diff_m=diff))
            print("repeat %d  B %3d  largest difference of the last positions: %.3g m" % (rep, B, diff), flush=True)
    # the SfM input: the 64 tables the last run left
    slots = list(range(64))
    for s in slots:
        if fh.counts(s)[0] == 0:                             # (a run with fewer than 64 drivers)
            t = fh.tracks_get(0)
            fh.tracks_set(s, t["ids"], t["start"], t["depth"], t["flag"], t["off"], t["pts"])
    one, many = [], []
    for r in range(args.reps + 2):
        for leg in (("batch", "loop") if r % 2 == 0 else ("loop", "batch")):
            t0 = time.perf_counter()
            if leg == "batch":
                fh.tracks_batch(slots)
            else:
                for s in slots:
                    fh.tracks_get(s)
            (one if leg == "batch" else many).append(1e3 * (time.perf_counter() - t0))
    tracks = dict(slots=64, tracks_per_slot=float(np.mean([fh.counts(s)[0] for s in slots])), tracks_batch_ms=float(np.median(one[2:])),
                  tracks_get_x64_ms=float(np.median(many[2:])))
    print("tracks: %(slots)d slots of %(tracks_per_slot).0f tracks  tracks_batch %(tracks_batch_ms).3f ms  64 x tracks_get %(tracks_get_x64_ms).3f ms" % tracks, flush=True)
    fh.close()
    res = dict(bench="stream_fm", frames=args.frames, repeats=args.repeats, reps=args.reps, rows=rows, tracks=tracks)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
