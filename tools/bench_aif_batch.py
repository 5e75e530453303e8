"""One INITIAL try of B streams whose all_image_frame holds 11 keyframes and 4 non-keyframes, 150 tracks and 20 IMU samples per
interval (tests/aif_scenes.py's "middle" window), from the SfM's result to the alignment's.

  leg batch  aif.initialize_from_frames over B resident slots: four library calls (vio_aif_structure_batch,
             vio_init_gyro_bias_batch, vio_aif_propagate_batch, vio_init_align_batch), DESIGN.md section 31
  leg loop   today's path from Python lists: pnp.pnp_items_from_sfm, PnpHandle.frames_batch, pnp.all_frames_to_init_items and
             InitHandle.initialize_batch (which loads the raw intervals into an ImuHandle and re-propagates them)

Both legs start from the same SfM results and end with the alignment's dicts.  Feeding the slots (leg batch) and keeping the lists
(leg loop) happen frame by frame while a stream runs and are outside the timed part of both.  Per leg and B: the wall time of a try,
the median of --reps tries after --warmup, with the least and the most.  The two legs of a B run back to back, and --repeats runs the
whole measurement again with the order of the legs alternating, for the spread.

    python tools/bench_aif_batch.py [--batches 1,64,256] [--reps 10] [--warmup 2] [--repeats 3] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import aif_reference as ar  # noqa: E402
import aif_scenes as sc  # noqa: E402

TIC, G_NORM = sc.TIC, 9.81


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    vio = g.load_package()
    ah, ih, ph, mh = vio.load_aif().create(), vio.load_init().create(), vio.load_pnp().create(), vio.load_imu().create()
    runs = []
    for B in [int(v) for v in a.batches.split(",")]:
        scenes = [sc.make("middle", seed=100 + i, n_tracks=150, dead=6, n_smp=20) for i in range(B)]
        refs = []
        for i, scn in enumerate(scenes):
            ah.reset(i)
            sc.feed(ah, i, scn)
            r = ar.ImageFramesReference()
            sc.feed(r, 0, scn)
            refs.append(r.frames_get(0))
        frames = vio.BatchImageFrames(ah, range(B))
        sfm = [dict(status=0, Q=s["item"]["Q"], T=s["item"]["T"], points=s["item"]["points"], state=s["item"]["state"]) for s in scenes]
        headers, tids = [s["item"]["headers"] for s in scenes], [s["item"]["track_ids"] for s in scenes]
        # the lists of leg loop: every frame's observations as the SfM item's tracks, the raw intervals, the records held on the host
        sfm_items = [dict(n_frames=11, start_frame=np.zeros(150, dtype=np.int32)) for _ in scenes]
        all_frames, ivs, pres = [], [], []
        st0 = frames.structure([dict(s["item"]) for s in scenes])
        for s, slot, o in zip(scenes, refs, st0):
            track = {int(v): k for k, v in enumerate(s["item"]["track_ids"].tolist())}
            fr = []
            for f, key in zip(slot["frames"], s["is_key"]):
                keep = [k for k, v in enumerate(f["ids"].tolist()) if v in track]
                fr.append(dict(is_key=key, obs_point=np.array([track[int(f["ids"][k])] for k in keep], dtype=np.int32), obs_pts=f["pts"][keep]))
            all_frames.append(fr)
            ivs.append(ar.intervals(slot))
            pres.append([o["preint"][j] for j in range(len(slot["frames"]) - 1)])
        is_key = [s["is_key"] for s in scenes]

        def leg_batch():
            return vio.initialize_from_frames(frames, ih, sfm, headers, tids, sc.RIC, TIC, G_NORM)

        def leg_loop():
            items = vio.pnp_items_from_sfm(sfm, sfm_items, all_frames)
            pnp = ph.frames_batch(items)
            init = vio.all_frames_to_init_items(sfm, pnp, sc.RIC, pres, is_key)
            return ih.initialize_batch(init, ivs, mh, TIC, G_NORM)

        x, y = leg_batch(), leg_loop()
        assert all(p["status"] == 0 and q["status"] == 0 for p, q in zip(x, y)), "a window was not aligned"       # the tries timed are ones that succeed
        assert all(np.allclose(p["bg"], q["bg"], rtol=0, atol=1e-9) for p, q in zip(x, y)), "the legs disagree"      # (R differs in its last bits)
        for rep in range(a.repeats):
            order = [("batch", leg_batch), ("loop", leg_loop)][::1 if rep % 2 == 0 else -1]
            for name, fn in order:
                t = []
                for k in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    fn()
                    t.append(1e3 * (time.perf_counter() - t0))
                t = t[a.warmup:]
                runs.append(dict(B=B, leg=name, repeat=rep, first=order[0][0], median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)))
                print(json.dumps(runs[-1]))
    out = dict(tool="bench_aif_batch", window="11 keyframes + 4 non-keyframes, 150 tracks, 20 samples per interval", reps=a.reps, warmup=a.warmup, runs=runs)
    summary = {}
    for B in sorted({r["B"] for r in runs}):
        summary[str(B)] = {leg: float(np.median([r["median_ms"] for r in runs if r["B"] == B and r["leg"] == leg])) for leg in ("batch", "loop")}
    out["median_of_medians_ms"] = summary
    print(json.dumps(summary))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
