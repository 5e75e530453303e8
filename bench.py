#!/usr/bin/env python3
"""bench.py — GN iterations/s of the MI355X sliding-window VIO backend on BASELINE.json's headline config.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--landmarks L] [--landmark-type invdepth|xyz] [--dump-outputs DIR] [--full]

One "step" = one Gauss-Newton iteration of the hot path: linearise all reprojection
+ IMU factors, reduce the landmark Schur complement, add the prior, damped pivoted LDLT of the 171x171 pose
system, back-substitute the landmarks, update every state, re-evaluate chi2 — `vio_gn_iteration` of
include/vio_backend.h, enqueued back to back with no host round trip.  Inputs are resident in HBM before the
timed region starts.

N = 1: the 11-frame / 20 000-landmark / 80 000-observation synthetic window (BASELINE.json configs[2]).
N > 1: BASELINE.json configs[3] — ONE 200 000-landmark / 800 000-observation window, its landmarks block-sharded over the N
       GPUs (25 000 per GPU at N = 8): strong scaling.  One process per GPU (torch.distributed, backend nccl == RCCL, for
       the rendezvous, the barriers and the 128-byte communicator id); per iteration the library itself issues ONE RCCL
       all-gather of the shards' 24 KB partial reduced systems on its stream and adds them in rank order (SURVEY.md
       section 8e).  `value` = GN iterations/s of THAT window (steps / elapsed — N ranks working on
       one iteration count once); with --full, `single_gpu_same_window_ms` is the same window unsharded on rank 0's GPU,
       measured in the same run, so the speed-up is in the line.
       Launch: `python bench.py --gpus N` spawns its N rank processes itself (the parent never touches a GPU), or
       `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N` (RANK / WORLD_SIZE from the environment).
       VIO_BENCH_ONE_DEVICE=1 puts every rank on device 0 with the exchange staged through host memory over gloo (RCCL
       refuses two ranks on one device): the N > 1 code path on a one-GPU box (tests/test_gpu_bench_launch.py).

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line.  Its JSON line also carries
  roofline      achieved = algorithmic bytes per launch / measured launch duration of the dominant kernel
                (HIP event pairs on the library's stream around about ten launches spread over the timed steps),
                peak = 8 TB/s HBM

--full adds, after the timed steps (each block can be left out with its --no-* / size option):
  cpu_baseline  the oracle's (oracle/vio_oracle.c, plain C, 1 thread) GN iteration on the same window, timed on the
                host on a bounded sample; with cpu_baseline_all_cores (OpenMP build) and cpu_reference (oracle/_ref)
  per_frame     what surrounds the inner iteration once per frame: vio_set_*, plan + upload + first linearisation,
                Solve(10), MargOldFrame — host wall clock, for the HIP library and for the CPU port; per_frame_small
                the same in the reference's regime (N = 150 / 300, the MH_05 real-IMU windows, four backends)
  scale_projection, batched (N = 1), single_gpu_same_window_ms and replicas (N > 1)
Without --full these keys are null.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(ROOT, "visual-inertial-odometry_amd")


def load_package():
    if "vio_amd" in sys.modules:
        return sys.modules["vio_amd"]
    spec = importlib.util.spec_from_file_location(
        "vio_amd", os.path.join(PKG_DIR, "__init__.py"), submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vio_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


CHAIN_IMAGE_BYTES = 16096 * 8        # CH_PACKED doubles (csrc/vio_pose_solve_chain.h): the tiles of the chain order + right-hand side
PAIR_TABLE_BYTES = (121 * 40 + 16) * 8    # the reprojection chains k_pose_solve leaves for the next linearisation
FP64_PEAK_TFLOPS = 78.6              # 1024 SIMDs x 32 FLOP/clk (v_mfma_f64_16x16x4_f64: 64 cycles; tools/microbench/mfma_lds_stream.hip) x 2.4 GHz = the vector fp64 rate


def algorithmic_flops(n, m):
    """SURVEY.md section 8(d), secondary figure: per observation ~150 (residual) + 600 (Jacobians) + 900 (weighted block products),
    per landmark ~930 (Schur rank-1 update on <= 30 columns): 7.5 kflop per landmark at 4 observations."""
    return 1650.0 * m + 930.0 * n


# algorithmic bytes of one launch of each kernel, N landmarks / M observations on this GPU
def kernel_algorithmic_bytes(name, n, m, xyz=False):
    if xyz:     # per observation (x, y) fp64 + 2 int32 of indices; per landmark 3 fp64 read, 3 fp64 written (+ 3 of delta)
        b_state, b_imu = 1464, 10 * (10 + 225 + 225 + 6 + 1) * 8
        b_sys = (171 * 171 + 171) * 8
        return {"k_linearize": 24 * m + 48 * n + b_state + b_imu, "k_reduce": 78 * 36 * 8 * 2, "k_assemble": 2 * b_sys,
                "k_pose_solve": 2 * b_sys + b_state + 171 * 8, "k_backsub": 24 * m + 72 * n + b_state, "k_lm_decide": 4096}[name]
    b_state = 1464
    b_imu = 10 * (10 + 225 + 225 + 6 + 1) * 8
    b_sys = (171 * 171 + 171) * 8
    return {
        # reads: 2 (x,y) fp64 per observation + per-landmark host (x,y) + inverse depth + 3 int32 of indices per
        # observation (44 B/obs + 8 B/landmark); writes h_ll/b_l per landmark
        "k_linearize": 44 * m + 16 * n + b_state + b_imu,
        "k_reduce": 78 * 36 * 8 * 2,
        "k_assemble": 2 * b_sys,
        "k_pose_solve": 2 * b_sys + b_state + 171 * 8,
        # reads pts (44 B/obs), inverse depth + writes the trial inverse depth and delta per landmark
        "k_backsub": 44 * m + 24 * n + b_state,
        "k_lm_decide": 4096,
    }[name]


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, ctx, xyz, chi2, rank, world, dist):
    """--dump-outputs DIR: what the timed path's last step hands a caller — the window's states, the landmarks, the step it took and the
    re-evaluated chi2 — as float64 .npy files, so that two builds run with the same arguments can be compared array for array.  N > 1:
    the landmark arrays are gathered over the ranks in rank order (the original landmark order) and rank 0 writes.  Landmark arrays
    larger than the 64 MB budget are replaced by a fixed, seeded sample of their rows (landmark_index.npy names the rows)."""
    import numpy as np
    poses, speed_bias, ext = ctx.get_window()
    dx_pose, dx_lm = ctx.get_delta()
    lms = ctx.get_landmarks_xyz() if xyz else ctx.get_landmarks()
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, (lms, dx_lm))
        lms = np.concatenate([p[0] for p in parts])
        dx_lm = np.concatenate([p[1] for p in parts])
    if rank != 0:
        return
    arrays = {"poses": poses, "speed_bias": speed_bias, "extrinsic": ext, "delta_pose": dx_pose, "chi2": np.array([chi2])}
    fixed = sum(a.nbytes for a in arrays.values())
    n = lms.shape[0]
    row_bytes = (lms.nbytes + dx_lm.nbytes) // max(n, 1)
    if fixed + n * row_bytes > DUMP_LIMIT_BYTES:
        k = (DUMP_LIMIT_BYTES - fixed) // (row_bytes + 8)
        idx = np.sort(np.random.RandomState(0).choice(n, k, replace=False))
        lms, dx_lm = lms[idx], dx_lm[idx]
        arrays["landmark_index"] = idx
    arrays["landmarks_xyz" if xyz else "landmarks_inv_depth"] = lms
    arrays["delta_landmarks"] = dx_lm
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N rank processes as children of this one — fresh interpreters,
    started before this process has made any GPU call (it never makes one) — hand them the torch.distributed environment, pass
    rank 0's stdout through, and leave with the first non-zero exit code."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    # poll all of them: a rank that dies leaves the others inside a collective, where they would sit until the backend's own
    # timeout — the first non-zero exit ends the rest within a second (waiting for the children in order blocked on rank 0)
    import time
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            r = p.poll()
            if r is None:
                continue
            live.remove(p)
            if r != 0 and rc == 0:
                rc = r
        if rc != 0:
            for p in live:
                p.terminate()
            t_end = time.time() + 5.0
            for p in live:
                try:
                    p.wait(timeout=max(0.1, t_end - time.time()))
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
            break
        if live:
            time.sleep(0.05)
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--landmarks", type=int, default=20000, help="landmarks of the N = 1 window")
    ap.add_argument("--landmarks-total", type=int, default=200000, help="landmarks of the window N > 1 GPUs share (BASELINE.json configs[3])")
    ap.add_argument("--obs-per-landmark", type=int, default=4)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prior", action="store_true", help="first-window case: no marginalisation prior")
    ap.add_argument("--landmark-type", choices=("invdepth", "xyz"), default="invdepth",
                    help="invdepth: VertexInverseDepth + EdgeReprojection (what Estimator builds, the headline); "
                         "xyz: VertexPointXYZ + EdgeReprojectionXYZ (3x3 landmark blocks)")
    ap.add_argument("--batch", type=int, default=64, help="windows of the batched block (vio_batch_gn_iteration); 0 skips it")
    ap.add_argument("--batch-full", type=int, default=256, help="windows of the batched block's full-device figure (one pose solve per CU); 0 skips it")
    ap.add_argument("--no-per-frame", action="store_true", help="skip the per-frame cost block (set / plan+upload / Solve(10) / marginalise)")
    ap.add_argument("--no-small-regime", action="store_true", help="skip the per_frame_small block (N = 150 / 300 and the MH_05 real-IMU windows, four backends)")
    ap.add_argument("--cpu-baseline-steps", type=int, default=0, help="0 = sized for about 10-20 s")
    ap.add_argument("--replica-windows", type=int, default=16, help="N > 1: independent windows per GPU of the `replicas` block (0 skips it)")
    ap.add_argument("--replica-landmarks", type=int, default=20000)
    ap.add_argument("--no-scale-projection", action="store_true", help="N = 1: skip the scale_projection block (the sharded launch sequence on the 200 000 / N-landmark shards of configs[3], one GPU)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure the CPU baselines, per-frame costs, scale projection, batched windows (N = 1) "
                         "and the unsharded / replicated windows (N > 1); a plain run measures the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step handed back (window, landmarks, step, chi2) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))          # before anything here has touched a GPU (torch is not even imported yet)
    # test hook of the launcher (tests/test_bench_launcher.py, no GPU needed): rank VIO_BENCH_FAIL_RANK leaves with code 3 at once, the
    # others sit still as if inside a collective — the parent has to end them
    if "VIO_BENCH_FAIL_RANK" in os.environ and "RANK" in os.environ:
        if os.environ["RANK"] == os.environ["VIO_BENCH_FAIL_RANK"]:
            sys.exit(3)
        time.sleep(600)
        sys.exit(0)

    import numpy as np
    import torch

    # The contract is ONE JSON line on stdout.  Libraries talk there too (RCCL prints its version banner on the C stdout when a communicator
    # is created, gloo its connections): from here to the final print file descriptor 1 is stderr, and the real stdout comes back — with the C
    # library's buffer flushed first — for that one line.
    sys.stdout.flush()
    real_stdout_fd = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    one_device = os.environ.get("VIO_BENCH_ONE_DEVICE") == "1"      # all ranks on device 0: the N > 1 path on a one-GPU box
    if one_device:
        local_rank = 0
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False (no CPU fallback exists)")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if one_device:      # RCCL refuses two ranks on one device: gloo for the rendezvous, the exchange through pinned host memory
            os.environ.setdefault("VIO_EXCHANGE", "hook_host")
            # (gloo announces its connections on the C++ stdout: keep this process's stdout for the one JSON line)
            sys.stdout.flush()
            keep = os.dup(1)
            os.dup2(2, 1)
            try:
                dist.init_process_group(backend="gloo")
                dist.barrier()
            finally:
                os.dup2(keep, 1)
                os.close(keep)
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))

    vio = load_package()
    hip = vio.load_hip()        # raises if csrc/libvio_hip.so is missing: no fallback path

    k_obs = args.obs_per_landmark
    n_total = args.landmarks if world == 1 else args.landmarks_total
    n_per_gpu = (n_total + world - 1) // world
    xyz = args.landmark_type == "xyz"
    make = vio.synth.make_window_xyz if xyz else vio.synth.make_window
    full = make(n_total, seed=42, obs_per_landmark=k_obs)
    if not args.no_prior:
        # the steady-state window carries a marginalisation prior ("produced by running one MargOldFrame
        # on a preceding window"; its 235 KB are part of B_win): solve the window one frame earlier, marginalise its
        # oldest frame (rank 0; the others receive the same bytes)
        prior = None
        if rank == 0:
            wp = vio.synth.make_window(300, seed=41, t0=0.9, obs_per_landmark=k_obs)
            cp = hip.context(device=local_rank)
            cp.load(wp)
            cp.solve(10)
            prior = cp.marginalize(vio.MARG_OLD)
            del cp
        if dist is not None:
            box = [prior]
            dist.broadcast_object_list(box, src=0)
            prior = box[0]
        full.prior = prior

    # N > 1: the library all-reduces with RCCL itself on its own stream (VIO_EXCHANGE=hook selects the
    # torch.distributed hook instead, which has to share torch's current stream)
    kw = dict(device=local_rank)       # (with VIO_EXCHANGE=hook, ShardedBackend puts the library and the collective on one torch stream)
    force = os.environ.get("VIO_BENCH_FORCE_EXCHANGE") == "1"      # diagnostic: run the sharded kernel sequence on one rank
    if force and dist is None and os.environ.get("VIO_EXCHANGE", "native") == "hook":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", local_rank))
    sb = vio.sharded.ShardedBackend(hip, full, rank, world, dist=dist, torch_device="cuda", ctx_kwargs=kw, force_hook=force)
    ctx, w = sb.ctx, sb.shard
    n, m = w.n_landmarks, w.n_observations

    # lambda of the reference's LM start (ComputeLambdaInitLM): identical on every rank after the exchange
    ctx.linearize()
    _, lam = ctx.init_lm()

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        ctx.gn_iteration(lam)
    ctx.synchronize()

    # which kernel dominates?  one short profiled pass per kernel (outside the timed region).  Every run makes it, --full or not: the
    # timed loop brackets the kernel it finds, and its iterations are part of the state the timed steps start from
    per_kernel = {}
    for kid, name in enumerate(hip.KERNELS):
        ctx.profile_begin(kid)
        for _ in range(10):
            ctx.gn_iteration(lam)
        ms, cnt = ctx.profile_end()
        per_kernel[name] = ms / max(cnt, 1)
    dominant = max(per_kernel, key=per_kernel.get)

    # timed region: exactly K steps; an event pair around every `stride`-th launch of the dominant kernel — about ten pairs
    # over the region, never fewer than every 8th launch (a hipEventRecord drains the stream, ~7 us each: bracketing every
    # launch would add ~15 % to the step it is meant to observe, every 8th still 2.5 %)
    stride = max(8, args.steps // 10)
    ctx.profile_begin_sampled(hip.KERNELS.index(dominant), stride)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ctx.gn_iteration(lam)
    ctx.synchronize()
    barrier()
    t1 = time.perf_counter()
    dom_ms, dom_cnt = ctx.profile_end()
    elapsed = t1 - t0
    if dist is not None:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if one_device else "cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    chi2 = ctx.chi2()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, ctx, xyz, chi2, rank, world, dist)
    ms_per_step = elapsed * 1e3 / args.steps
    value = args.steps / elapsed            # iterations of THE window per second: N ranks working on one iteration count once

    # N > 1: the same window unsharded on rank 0's GPU, in the same run (the others wait at the barrier)
    single_gpu = None
    if world > 1 and args.full:
        if rank == 0:
            c1 = hip.context(device=local_rank)
            c1.load(full)
            c1.linearize()
            _, lam1 = c1.init_lm()
            for _ in range(10):
                c1.gn_iteration(lam1)
            c1.synchronize()
            n1 = max(20, min(args.steps, 100))
            t = time.perf_counter()
            for _ in range(n1):
                c1.gn_iteration(lam1)
            c1.synchronize()
            single_gpu = (time.perf_counter() - t) * 1e3 / n1
            del c1
        barrier()

    # N > 1, the regime that scales: every GPU runs its own batch of independent windows (vio_batch_gn_iteration), no collective in
    # the data path; the job's figure is the sum over the ranks of windows x iterations / the slowest rank's time
    replicas = None
    if world > 1 and args.full and args.replica_windows > 0:
        rw, rn = args.replica_windows, args.replica_landmarks
        rkw = dict(device=local_rank, item_policy=vio.capi.ITEMS_THROUGHPUT)
        lead = hip.context(**rkw)
        rkw["stream"] = lead.get_stream()
        members = [lead] + [hip.context(**rkw) for _ in range(rw - 1)]
        for i, cx in enumerate(members):
            cx.load(make(rn, seed=1000 + 97 * rank + i, obs_per_landmark=k_obs))
        for _ in range(3):
            hip.batch_gn_iteration(members, lam)
        lead.synchronize()
        barrier()
        t = time.perf_counter()
        rsteps = 20
        for _ in range(rsteps):
            hip.batch_gn_iteration(members, lam)
        lead.synchronize()
        barrier()
        rel = time.perf_counter() - t
        tt = torch.tensor([rel], dtype=torch.float64, device="cpu" if one_device else "cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        rel = float(tt.item())
        replicas = {"windows_per_gpu": rw, "landmarks_per_window": rn, "steps": rsteps,
                    "window_iterations_per_s": world * rw * rsteps / rel, "us_per_window_iteration_per_gpu": rel * 1e6 / (rw * rsteps),
                    "scaling": "weak", "note": "independent windows, one batch per GPU, no collective in the data path"}
        del members, lead

    dom_launch_s = (dom_ms / max(dom_cnt, 1)) * 1e-3
    alg_bytes = kernel_algorithmic_bytes(dominant, n, m, xyz)
    # the kernel's symbol as rocprofv3 lists it: with the chain order (the default) the sums and the solve run as
    # k_reduce_c / k_pose_solve_c, and the solve reads the 120 KB chain image instead of the 235 KB dense system
    chain = ctx.get_solve_order()[1] == vio.capi.ORDER_CHAIN
    symbol = dominant + ("_c" if chain and dominant in ("k_reduce", "k_pose_solve") else "") + ("_xyz" if xyz and dominant == "k_linearize" else "")
    if chain and dominant == "k_pose_solve":
        alg_bytes = CHAIN_IMAGE_BYTES + 1464 + 171 * 8 + (0 if xyz else PAIR_TABLE_BYTES)
    achieved = alg_bytes / dom_launch_s / 1e9 if dom_launch_s > 0 else 0.0
    # HBM bytes per launch: NOT measured in this run (PMC counters need rocprofv3 around the process): the figure of the
    # committed counter pass over this same command (profiles/traffic.json <- tools/summarize_profile.py), labelled as such
    traffic, traffic_source = None, None
    tr_path = os.path.join(ROOT, "profiles", "traffic_xyz.json" if xyz else "traffic.json")
    if os.path.exists(tr_path):
        try:
            traffic = json.load(open(tr_path)).get(symbol, {}).get("hbm_bytes_per_launch")
            traffic_source = "committed rocprofv3 --pmc pass (profiles/%s), not this run" % os.path.basename(tr_path)
        except Exception:
            traffic = None
    it_bytes = (24 * m + 72 * n + 280000) if xyz else vio.synth.algorithmic_bytes(n, m)
    # Which roof?  k_pose_solve(_c) is ONE workgroup on one of the device's CUs walking a dependent chain of pivots: neither the HBM roof
    # nor the device's fp64 roof binds it ("latency"); its arithmetic against ONE CU's fp64 rate is given beside the HBM fraction
    # (171^3 / 3 flops, the dense LDL^T's count, as the upper bound of what the structured solve performs).  k_linearize: nearer the fp64
    # matrix roof than the HBM one (14 % against 3.5 % for one window, 22 % against 5.5 % batched).
    n_cus_dev = torch.cuda.get_device_properties(0 if one_device else local_rank).multi_processor_count
    if dominant == "k_pose_solve":
        bound = "latency"
        flops = 171.0 ** 3 / 3.0
        fp64 = {"flops_per_launch_upper_bound": flops, "one_cu_peak_GFLOPs": round(FP64_PEAK_TFLOPS * 1e3 / n_cus_dev, 1),
                "achieved_GFLOPs": round(flops / dom_launch_s / 1e9, 2) if dom_launch_s > 0 else 0.0,
                "frac_of_one_cu": (flops / dom_launch_s / 1e9) / (FP64_PEAK_TFLOPS * 1e3 / n_cus_dev) if dom_launch_s > 0 else 0.0,
                "workgroups": 1, "cus_of_the_device": n_cus_dev}
    elif dominant == "k_linearize":
        bound = "mfma"
        flops = algorithmic_flops(n, m)
        fp64 = {"algorithmic_flops_per_launch": flops, "peak_TFLOPs": FP64_PEAK_TFLOPS,
                "achieved_TFLOPs": round(flops / dom_launch_s / 1e12, 3) if dom_launch_s > 0 else 0.0,
                "frac": (flops / dom_launch_s / 1e12) / FP64_PEAK_TFLOPS if dom_launch_s > 0 else 0.0}
    else:
        bound, fp64 = "latency", None
    roofline = {"bound": bound, "kernel": symbol, "achieved": round(achieved, 3), "peak": 8000.0, "unit": "GB/s",
                "frac": achieved / 8000.0, "fp64": fp64, "traffic": traffic, "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": alg_bytes, "launch_us": round(dom_launch_s * 1e6, 3),
                "launch_us_method": "HIP event pairs on the library's stream around every %d-th launch of the timed steps " % stride +
                                    "(includes the event's own drain, ~8 % above rocprofv3's kernel duration)",
                "iteration_algorithmic_bytes": it_bytes,
                "iteration_achieved_GBps": round(it_bytes / (ms_per_step * 1e-3) / 1e9, 3),
                "kernel_us_event_bracketed": {k: round(v * 1e3, 3) for k, v in per_kernel.items()}}

    # ---- what one frame costs around the inner iteration (Estimator::backendOptimization, estimator.cpp:1075-1141):
    #      vio_set_* of a fresh window, plan + upload + first linearisation, Solve(10), MargOldFrame — host wall clock
    per_frame = None
    if rank == 0 and world == 1 and args.full and not args.no_per_frame:
        # a stream of windows, one frame (0.1 s) apart on the generator's trajectory, each with fresh landmarks: frame r + 1 is set with
        # THE PRIOR FRAME r's MargOldFrame RETURNED (estimator.cpp:693-901 -> :1020-1034), so vio_set_prior copies and uploads its
        # 430 KB in every timed frame (round 3 alternated two windows that shared one prior, and the library's keep-if-equal test
        # skipped that copy: VERDICT r03 weak #7)
        n_stream = 22
        stream_w = [full] + [make(n_per_gpu, seed=42 + r, obs_per_landmark=k_obs, t0=1.0 + 0.1 * r) for r in range(1, n_stream)]

        def stats(v):
            v = sorted(v)
            return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}

        def frame_costs(lib, reps, warm=2, windows=None, pipelined=False, ctx_kw=None):
            """`reps` timed frames after `warm` untimed ones (one per window: first touches, buffers reaching their size).
            A frame never repeats the one before (the library skips inputs it already holds).
            pipelined: MargOldFrame as vio_marginalize_begin; its dense host tail runs on the library's helper thread under the next
            frame's vio_set_window / landmarks / observations / imu and is collected (vio_marginalize_end) in front of vio_set_prior."""
            wins = windows or stream_w
            for w_ in wins:         # (a caller holds its pre-integrations as vio_preint structs: the dict -> struct conversion of the generator is not a frame's cost)
                w_.preint = [p_ if (p_ is None or isinstance(p_, vio.VioPreint)) else vio.VioPreint.from_dict(p_) for p_ in w_.preint]
            chain = not xyz         # (XYZ graphs have no MargOldFrame caller: their windows keep the prior they came with)
            next_prior = wins[0].prior
            c = lib.context(**dict({"device": local_rank} if lib is hip else {}, **(ctx_kw or {})))
            phases = ("set_ms", "plan_upload_linearize_ms", "solve10_ms", "marginalize_ms")
            acc = {k: [] for k in phases}
            acc["frame_ms"] = []
            split = {"marg_device_us": [], "marg_tail_us": [], "marg_prepare_us": [], "activate_plan_us": [], "activate_push_us": []}
            iters = live = 0
            for r in range(reps + warm):
                t0 = time.perf_counter()
                wr = wins[r % len(wins)]
                if pipelined:
                    c.set_window(wr.poses, wr.speed_bias, wr.ext)
                    c.set_landmarks(wr.inv_depth)
                    c.set_observations(wr.lm, wr.host, wr.target, wr.pts_i, wr.pts_j)
                    c.set_imu_all(wr.preint)
                    c.prepare()             # (vio_prepare: the plan of the new graph built and uploaded while the tail still runs)
                    if r > 0:
                        next_prior = c.marginalize_end()
                    c.set_prior(next_prior if chain else wr.prior)
                else:
                    if chain:
                        wr.prior = next_prior
                    c.load(wr)
                t1 = time.perf_counter()
                c.linearize()
                if lib is hip:
                    c.synchronize()
                    ht_a = c.host_timing()
                t2 = time.perf_counter()
                rep = c.solve(10)
                t3 = time.perf_counter()
                t4 = t3
                if not xyz:
                    if pipelined:
                        c.marginalize_begin(vio.MARG_OLD)
                    else:
                        next_prior = c.marginalize(vio.MARG_OLD)
                    t4 = time.perf_counter()
                if r < warm:
                    continue
                for k, v in zip(phases, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    acc[k].append(v * 1e3)
                acc["frame_ms"].append((t4 - t0) * 1e3)
                iters = rep.iterations
                if lib is hip:
                    ht = c.host_timing()
                    for k in ("marg_device_us", "marg_tail_us", "marg_prepare_us"):
                        split[k].append(ht[k])
                    for k in ("activate_plan_us", "activate_push_us"):
                        split[k].append(ht_a[k])
                    live = int(ht["marg_live_rows"])
            if pipelined:
                c.marginalize_end()
            out = {k: stats(v)["median"] for k, v in acc.items()}
            out["spread"] = {k: stats(v) for k, v in acc.items()}
            out["solve10_iterations"] = iters
            if lib is hip:
                out["host_split_us_median"] = {k: stats(v)["median"] for k, v in split.items()}
                out["marginalize_live_rows_of_156"] = live
            if xyz:
                out["marginalize_ms"] = None
            return out

        per_frame = {"gpu": frame_costs(hip, 20),
                     "note": "host wall clock per call on the bench window, median of 20 frames (spread: min / max); set = "
                             "vio_set_window/landmarks/observations/imu/prior (host copies), plan_upload_linearize = pattern grouping + "
                             "H2D + first linearisation, marginalize = MargOldFrame: GPU assembly + Schur, 171x171 D2H (marg_device_us), "
                             "eigen-decomposition tail on one host thread (marg_tail_us; its plan is built under the solve: marg_prepare_us)"}
        if not xyz:
            pf = frame_costs(hip, 20, pipelined=True)
            per_frame["gpu_marginalisation_tail_in_the_background"] = {k: pf[k] for k in ("set_ms", "plan_upload_linearize_ms", "solve10_ms", "marginalize_ms", "frame_ms", "spread")}
        if not xyz:
            # MargOldFrame's worst case: tracks that span all frames — every frame-0 landmark seen from frames 1..10 — and a prior of
            # the same kind.  75 of the 156 rows of the reduced system are live then, and that is the most there can be: ext (6) + the ten
            # remaining poses (60) + the speed-bias of the FIRST remaining frame (9) — a speed-bias gets information from IMU factors
            # only, MargOldFrame's graph holds the one between frames 0 and 1 (estimator.cpp:735-747), and the prior it leaves hands
            # that block on to the next marginalisation: the other nine speed-bias blocks of a prior are exactly zero, always
            wd = [vio.synth.make_window(2000, seed=51 + r_, t0=1.0 + 0.1 * r_, obs_per_landmark=10) for r_ in range(n_stream)]
            # (a prior reaches the speed-bias rows of a frame only through the IMU edge 0 -> 1 of the marginalisation that removed the
            # frame before it: a chain of 11 marginalisations, each handing its prior to the next window, fills all of them)
            cpd = hip.context(device=local_rank)
            pd_ = None
            for q in range(11):
                wq = vio.synth.make_window(300, seed=60 + q, t0=-0.1 + 0.1 * q, obs_per_landmark=10)
                wq.prior = pd_
                cpd.load(wq)
                cpd.solve(10)
                pd_ = cpd.marginalize(vio.MARG_OLD)
            del cpd
            wd[0].prior = pd_           # (the frames after it take the prior their predecessor's MargOldFrame returns)
            dense = frame_costs(hip, 20, windows=wd)
            dense_bg = frame_costs(hip, 20, windows=wd, pipelined=True)
            per_frame["dense_prior"] = {"marginalize_ms_dense_prior": dense["marginalize_ms"], "spread": dense["spread"]["marginalize_ms"],
                                        "marginalize_ms_dense_prior_tail_in_the_background": dense_bg["marginalize_ms"],
                                        "frame_ms": dense["frame_ms"], "frame_ms_tail_in_the_background": dense_bg["frame_ms"],
                                        "host_split_us_median": dense["host_split_us_median"],
                                        "marginalize_live_rows_of_156": dense["marginalize_live_rows_of_156"],
                                        "window": "a stream of windows of 2000 landmarks hosted in frame 0, each observed in frames 1..10; the first prior = the end of a chain of 11 such windows, each marginalised into the next, and every timed frame is set with the prior its predecessor returned"}

    # ---- the reference's real regime: NUM_OF_F = 1000 and ~150 tracked features make N = 100 .. 300 the only sizes
    #      Estimator can reach (VM/include/parameters.h:37).  Streams of ragged-track windows with chained priors at N = 150 and 300, and the
    #      windows a stream on the reference's own EuRoC MH_05 IMU data produces (real inertial data, synthetic vision): one frame =
    #      vio_set_*, first linearisation, Solve(10), MargOldFrame — through the HIP library (ctypes), through the C++ host mirror of
    #      Estimator::backendOptimization, through the CPU port, and through the COMPILED REFERENCE's own Problem::Solve(10) + Marginalize
    #      (oracle/_ref/libvio_ref.so, when the repo was built where /root/reference exists) on the same windows on this box's host.
    per_frame_small = None
    if per_frame is not None and not xyz and not args.no_small_regime:
        import subprocess
        per_frame_small = {"note": "host wall clock per frame, median of 20 frames (spread: min / max); the same windows for every backend; "
                                   "reference_compiled = the reference's own backend sources compiled where they lie (oracle/Makefile), 1 thread"}
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
        orc_s = vio.VioLib(os.path.join(ROOT, "oracle", "liboracle.so"), "vioo_")
        ref_path = os.path.join(ROOT, "oracle", "_ref", "libvio_ref.so")
        ref_s = vio.VioLib(ref_path, "vior_") if os.path.exists(ref_path) else None
        keys = ("set_ms", "plan_upload_linearize_ms", "solve10_ms", "marginalize_ms", "frame_ms", "spread", "solve10_iterations")

        def three_ways(wins, ctx_kw=None, reps=20):
            e = {"landmarks_median": int(np.median([w_.n_landmarks for w_ in wins])), "observations_median": int(np.median([w_.n_observations for w_ in wins]))}
            g = frame_costs(hip, reps, windows=[w_.copy() for w_ in wins], ctx_kw=ctx_kw)
            e["gpu_ctypes"] = {k: g[k] for k in keys}
            e["gpu_ctypes"]["host_split_us_median"] = g["host_split_us_median"]        # marg_device / marg_tail / marg_prepare / activate_* (us)
            e["gpu_ctypes"]["marginalize_live_rows_of_156"] = g["marginalize_live_rows_of_156"]
            gb = frame_costs(hip, reps, windows=[w_.copy() for w_ in wins], pipelined=True, ctx_kw=ctx_kw)
            e["gpu_ctypes_tail_in_the_background"] = {k: gb[k] for k in ("frame_ms", "spread")}
            o = frame_costs(orc_s, reps, warm=1, windows=[w_.copy() for w_ in wins], ctx_kw=ctx_kw)
            e["cpu_port_1_thread"] = {k: o[k] for k in keys}
            if ref_s is not None:
                try:
                    r_ = frame_costs(ref_s, reps, warm=1, windows=[w_.copy() for w_ in wins], ctx_kw=ctx_kw)
                    e["reference_compiled_1_thread"] = {k: r_[k] for k in keys}
                    e["frame_speedup_vs_reference_compiled"] = r_["frame_ms"] / g["frame_ms"]
                except Exception as exc:
                    e["reference_compiled_1_thread"] = {"error": str(exc)}
            return e

        for n_s in (150, 300):
            wins = [vio.synth.make_window(n_s, seed=300 + r_, t0=1.0 + 0.1 * r_, ragged=True) for r_ in range(22)]
            e = three_ways(wins)
            # the C++ host mirror (host/estimator_backend.cpp over the C ABI; tests/cpp/adapter_main.cpp timed inside the C++ program)
            try:
                outc = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_cpp_frame.py"), str(n_s), "20"], capture_output=True, text=True, timeout=300)
                for ln in outc.stdout.splitlines():
                    if ln.startswith("cpp_frame "):
                        tok = ln.split()
                        kv = {tok[i]: float(tok[i + 1]) for i in range(1, len(tok) - 1, 2)}
                        e.setdefault("gpu_cpp_mirror", {}).update(kv)
                if "gpu_cpp_mirror" not in e:
                    e["gpu_cpp_mirror"] = {"error": (outc.stderr or outc.stdout)[-300:]}
            except Exception as exc:
                e["gpu_cpp_mirror"] = {"error": str(exc)}
            per_frame_small["n%d" % n_s] = e
        # real inertial data: the windows a stream on the MH_05 stretch goes through (recorded from a run of the stream driver on the HIP library)
        try:
            zmh = dict(np.load(os.path.join(ROOT, "tests", "golden", "mh05_imu_stretch.npz")))
            st_mh = vio.stream.RealImuStream(zmh, landmarks_per_frame=30, seed=7)
            drv = vio.stream.StreamDriver(hip, st_mh, seed=2, ctx_kwargs={"device": local_rank})
            rec = []
            while True:
                drv.ensure_depths()
                rec.append(drv.window_arrays()[0])
                if not drv.step():
                    break
            for w_ in rec:
                w_.prior = None         # (every backend chains its own priors from frame to frame, as in the synthetic streams)
            per_frame_small["mh05_real_imu"] = three_ways(rec, ctx_kw={"gravity": (0.0, 0.0, st_mh.g_norm)}, reps=min(20, len(rec) - 2))
            per_frame_small["mh05_real_imu"]["frames_recorded"] = len(rec)
        except Exception as exc:
            per_frame_small["mh05_real_imu"] = {"error": str(exc)}

    # ---- N = 1: what a multi-GPU run of BASELINE.json configs[3] can be, MEASURED on this one GPU (the driver's
    #      scaling run keeps being skipped, so this is the scaling evidence a one-GPU driver can reproduce).  For N in {2, 4, 8}: the shard
    #      rank 0 would hold — 200 000 / N landmarks of the shared window with all their observations — through the SHARDED launch sequence
    #      (k_linearize -> k_reduce -> ncclAllGather -> k_assemble_c -> k_pose_solve_c, the library's own RCCL exchange on a one-rank
    #      communicator: the collective's launch is in the figure, its xGMI latency between real ranks is not), against the whole window
    #      unsharded (three launches) in the same run.  projected_speedup = unsharded / shard: an UPPER bound.
    scale_projection = None
    if rank == 0 and world == 1 and not xyz and args.full and not args.no_scale_projection:
        try:
            n_sp = args.landmarks_total
            big = make(n_sp, seed=42, obs_per_landmark=k_obs)
            big.prior = full.prior

            def gn_ms(backend_ctx, steps_sp=60, warm_sp=10):
                backend_ctx.linearize()
                _, lam_sp = backend_ctx.init_lm()
                for _ in range(warm_sp):
                    backend_ctx.gn_iteration(lam_sp)
                backend_ctx.synchronize()
                t_sp = time.perf_counter()
                for _ in range(steps_sp):
                    backend_ctx.gn_iteration(lam_sp)
                backend_ctx.synchronize()
                return (time.perf_counter() - t_sp) * 1e3 / steps_sp

            cu = hip.context(device=local_rank)
            cu.load(big)
            t_un = gn_ms(cu)
            del cu
            shards = {}
            for n_sh in (2, 4, 8):
                sh = vio.synth.shard_window(big, 0, n_sh)
                sbp = vio.sharded.ShardedBackend(hip, sh, 0, 1, dist=None, torch_device="cuda", ctx_kwargs=dict(device=local_rank), force_hook=True,
                                                 exchange=os.environ.get("VIO_EXCHANGE", "native"))
                t_sh = gn_ms(sbp.ctx)
                seen = sbp.ctx.comm_info()[0] if sbp.exchange == "native" else 0
                shards[str(n_sh)] = {"landmarks_per_gpu": sh.n_landmarks, "observations_per_gpu": sh.n_observations, "ms_per_iteration_per_shard": round(t_sh, 5),
                                     "projected_speedup": round(t_un / t_sh, 3), "exchange": sbp.exchange, "rccl_ranks_seen": seen}
                del sbp
            scale_projection = {
                "window": "BASELINE.json configs[3]: %d landmarks x %d observations, 10 IMU factors, prior" % (n_sp, k_obs),
                "unsharded_ms_per_iteration": round(t_un, 5), "shards": shards,
                "excluded": "the all-gather's latency between real ranks over xGMI (24 KB per rank: latency-bound) and the wait for the slowest rank",
                "note": "measured on ONE GPU: rank 0's shard through the sharded four-launch sequence (one-rank RCCL all-gather included) against the "
                        "unsharded window; the replicated part (k_assemble_c + k_pose_solve_c, ~32 us) bounds one window's strong scaling at "
                        "about 2.3x whatever the GPU count — the north star's >= 6x at 8 GPUs is out of reach by construction for ONE window; what "
                        "scales with GPUs is independent windows (the N > 1 line's `replicas` block, no collective)"}
        except Exception as exc:
            scale_projection = {"error": str(exc)}

    # ---- B independent windows per launch (vio_batch_gn_iteration): the regime in which the device is full.  Same window
    #      size as the headline, different seeds; reported beside the single-window line, never instead of it
    batched = None
    if rank == 0 and world == 1 and args.full and args.batch > 0:
        B = args.batch
        # (many windows share the device: items as large as the LDS holds, vio_config.item_policy)
        lead = hip.context(device=local_rank, item_policy=vio.capi.ITEMS_THROUGHPUT)
        members = [lead] + [hip.context(device=local_rank, stream=lead.get_stream(), item_policy=vio.capi.ITEMS_THROUGHPUT) for _ in range(B - 1)]
        wbs = []
        for i, cb in enumerate(members):
            wb = (vio.synth.make_window_xyz if xyz else vio.synth.make_window)(n_per_gpu, seed=100 + i, obs_per_landmark=k_obs)
            wb.prior = full.prior
            cb.load(wb)
            wbs.append(wb)
        for _ in range(5):
            hip.batch_gn_iteration(members, lam)
        lead.synchronize()
        bsteps = max(20, args.steps // 4)
        tb = time.perf_counter()
        for _ in range(bsteps):
            hip.batch_gn_iteration(members, lam)
        lead.synchronize()
        tb = time.perf_counter() - tb
        bytes_it = it_bytes        # (the window kind's own count: XYZ windows move 24 M + 72 N + B_win)

        def batched_roofline(group, nwin, nsteps):
            """k_linearize_hb (85 % of a batch iteration) against BOTH roofs: event pairs around every 8th of its launches in a pass
            of its own (not in the timed loop above), algorithmic bytes and flops of SURVEY.md 8(d) per launch, and the committed
            counter passes over the 64-window loop (tools/profile_batched.sh -> profiles/traffic_batched.json, *_batched_mfma.csv)
            scaled per window: HBM bytes actually moved, fp64 operations actually issued."""
            lead.profile_begin_sampled(0, 8)
            for _ in range(nsteps):
                hip.batch_gn_iteration(group, lam)
            ms, cnt = lead.profile_end()
            if cnt == 0:
                return None
            launch_s = ms / cnt * 1e-3
            name = "k_linearize_xyz_hb" if xyz else "k_linearize_hb"
            alg_b = nwin * kernel_algorithmic_bytes("k_linearize", n_per_gpu, full.n_observations, xyz)
            alg_f = nwin * algorithmic_flops(n_per_gpu, full.n_observations)
            out = {"kernel": name, "launch_us": round(launch_s * 1e6, 2), "launch_us_method": "HIP event pairs on the batch's stream around every 8th launch, %d pairs" % cnt,
                   "algorithmic_bytes_per_launch": alg_b, "algorithmic_flops_per_launch": alg_f,
                   "hbm_algorithmic_frac": alg_b / launch_s / 8e12, "fp64_algorithmic_frac": alg_f / launch_s / (FP64_PEAK_TFLOPS * 1e12)}
            try:        # counters: not this run (PMC needs rocprofv3 around the process); per window of the committed 64-window pass
                tr = json.load(open(os.path.join(ROOT, "profiles", "traffic_batched.json")))
                per_win = tr[name]["hbm_bytes_per_launch"] / tr.get("_windows", 64)
                out["traffic"] = nwin * per_win
                out["hbm_measured_traffic_frac"] = nwin * per_win / launch_s / 8e12
                ops = tr.get("_fp64", {}).get(name)
                if ops:
                    out["fp64_issued_flops_per_launch"] = nwin * ops["flops_per_launch"] / tr.get("_windows", 64)
                    out["fp64_issued_frac"] = out["fp64_issued_flops_per_launch"] / launch_s / (FP64_PEAK_TFLOPS * 1e12)
                    out["mfma_issued_frac"] = nwin * ops["mfma_flops_per_launch"] / tr.get("_windows", 64) / launch_s / (FP64_PEAK_TFLOPS * 1e12)
                out["counter_source"] = "committed rocprofv3 --pmc passes over tools/diag_batch_gn_timing.py 64 20000 (profiles/traffic_batched.json), per window; not this run"
            except Exception:
                out["traffic"] = None
            fr = {"hbm": max(out["hbm_algorithmic_frac"], out.get("hbm_measured_traffic_frac") or 0.0),
                  "mfma": max(out["fp64_algorithmic_frac"], out.get("fp64_issued_frac") or 0.0)}
            out["bound"] = max(fr, key=fr.get)
            if out["bound"] == "mfma":
                out.update(achieved=round(alg_f / launch_s / 1e12, 3), peak=FP64_PEAK_TFLOPS, unit="TFLOP/s", frac=out["fp64_algorithmic_frac"])
            else:
                out.update(achieved=round(alg_b / launch_s / 1e9, 2), peak=8000.0, unit="GB/s", frac=out["hbm_algorithmic_frac"])
            out["note"] = ("bound = the roof the kernel is nearer to, taking for each roof the larger of its algorithmic and its measured (issued / moved) "
                           "fraction; achieved / frac are the ALGORITHMIC figure on that roof; fp64 peak %.1f TFLOP/s = 32 FLOP/clk/SIMD measured" % FP64_PEAK_TFLOPS)
            return out

        batched = {"windows": B, "steps": bsteps, "ms_per_batch_iteration": tb * 1e3 / bsteps,
                   "window_iterations_per_s": B * bsteps / tb, "us_per_window_iteration": tb * 1e6 / (bsteps * B),
                   "algorithmic_GBps": round(B * bytes_it * bsteps / tb / 1e9, 2), "hbm_frac": B * bytes_it * bsteps / tb / 8e12,
                   "final_chi2_window0": lead.chi2(),
                   "note": "B independent 20k-landmark windows (seeds 100..), one launch per kernel for all of them (grid.y = window), contexts "
                           "created with item_policy = VIO_ITEMS_THROUGHPUT; bit-identical to B separate vio_gn_iteration runs of such contexts "
                           "(tests/test_gpu_batch.py)"}
        batched["roofline"] = batched_roofline(members, B, max(16, bsteps))
        # Problem::Solve(10) of the same B windows in one batched call (vio_batch_solve), from their initial states; the uploads
        # in front of it are not timed (per_frame has those)
        ts, its = [], 0
        for _ in range(3):
            for cb, wb in zip(members, wbs):
                cb.load(wb)
                cb.linearize()
            lead.synchronize()
            tb0 = time.perf_counter()
            reps_b = hip.batch_solve(members, 10)
            ts.append(time.perf_counter() - tb0)
            its = sum(r.iterations for r in reps_b) / len(reps_b)
        batched["solve10_ms_per_batch"] = min(ts) * 1e3
        batched["solve10_ms_per_window"] = min(ts) * 1e3 / B
        batched["solve10_mean_iterations"] = its
        # the same with one window per CU (k_pose_solve_b is one workgroup per window: 64 windows leave 192 CUs idle for 40 us of every
        # batch iteration); the extra contexts hold copies of the same 64 windows' data
        extra = []
        if args.batch_full > B:
            Bf = args.batch_full
            extra = [hip.context(device=local_rank, stream=lead.get_stream(), item_policy=vio.capi.ITEMS_THROUGHPUT) for _ in range(Bf - B)]
            for cb, wb in zip(members, wbs):
                cb.load(wb)
            for i, cb in enumerate(extra):
                cb.load(wbs[i % B])
            allm = members + extra
            for _ in range(3):
                hip.batch_gn_iteration(allm, lam)
            lead.synchronize()
            fsteps = max(10, bsteps // 2)
            tb = time.perf_counter()
            for _ in range(fsteps):
                hip.batch_gn_iteration(allm, lam)
            lead.synchronize()
            tb = time.perf_counter() - tb
            batched["full_device"] = {"windows": Bf, "steps": fsteps, "ms_per_batch_iteration": tb * 1e3 / fsteps,
                                      "window_iterations_per_s": Bf * fsteps / tb, "us_per_window_iteration": tb * 1e6 / (fsteps * Bf),
                                      "algorithmic_GBps": round(Bf * bytes_it * fsteps / tb / 1e9, 2), "hbm_frac": Bf * bytes_it * fsteps / tb / 8e12}
            batched["full_device"]["roofline"] = batched_roofline(allm, Bf, max(16, fsteps))
            del allm
        del cb, extra, members, lead          # (members first: they run on the leader's stream)

    cpu_baseline = None
    if rank == 0 and world > 1 and args.full and not args.no_cpu_baseline:
        # the CPU port on the WHOLE window the ranks share (the reference's dense solver would need 320 GB for it): a bounded sample
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
        orc = vio.VioLib(os.path.join(ROOT, "oracle", "liboracle.so"), "vioo_")
        co = orc.context()
        co.load(full)
        co.gn_iteration(lam)
        t = time.perf_counter()
        co.gn_iteration(lam)
        one = time.perf_counter() - t
        steps = args.cpu_baseline_steps or max(2, min(100, int(12.0 / max(one, 1e-3))))
        t = time.perf_counter()
        for _ in range(steps):
            co.gn_iteration(lam)
        dt = time.perf_counter() - t
        cpu_baseline = {"value": steps / dt, "unit": "GN iter/s", "cores": 1, "kind": "port", "ms_per_iter": dt * 1e3 / steps,
                        "sample": "%d GN iterations of the whole %d-landmark / %d-observation window the %d ranks share, "
                                  "oracle/vio_oracle.c (plain C, -O2, 1 thread), rank 0's host" % (steps, full.n_landmarks, full.n_observations, world)}
        del co
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
        orc = vio.VioLib(os.path.join(ROOT, "oracle", "liboracle.so"), "vioo_")
        if per_frame is not None:
            per_frame["cpu_port_1_thread"] = frame_costs(orc, 1, warm=1)
        co = orc.context()
        co.load(full)
        co.gn_iteration(lam)        # warm-up / first touch
        t = time.perf_counter()
        co.gn_iteration(lam)
        one = time.perf_counter() - t
        steps = args.cpu_baseline_steps or max(3, min(200, int(12.0 / max(one, 1e-3))))
        t = time.perf_counter()
        for _ in range(steps):
            co.gn_iteration(lam)
        dt = time.perf_counter() - t
        cpu_baseline = {"value": steps / dt, "unit": "GN iter/s", "cores": 1, "kind": "port",
                        "ms_per_iter": dt * 1e3 / steps,
                        "sample": "%d GN iterations of the same %d-landmark / %d-observation window, oracle/vio_oracle.c "
                                  "(plain C, -O2, 1 thread)" % (steps, n, m)}

    # the same port on all host cores (OpenMP over landmarks, oracle/liboracle_omp.so; SURVEY.md 8d asks for both figures)
    cpu_baseline_all_cores = None
    if cpu_baseline is not None and not xyz:       # (the OpenMP build parallelises the inverse-depth path only)
        try:
            import subprocess
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "omp"])
            omp = vio.VioLib(os.path.join(ROOT, "oracle", "liboracle_omp.so"), "vioo_")
            cm = omp.context()
            cm.load(full)
            cm.gn_iteration(lam)
            t = time.perf_counter()
            cm.gn_iteration(lam)
            one = time.perf_counter() - t
            steps = max(3, min(300, int(6.0 / max(one, 1e-3))))
            t = time.perf_counter()
            for _ in range(steps):
                cm.gn_iteration(lam)
            dt = time.perf_counter() - t
            navail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            ncores = min(16, navail)           # oracle_threads(): one window's work saturates at about 16 threads
            cpu_baseline_all_cores = {"value": steps / dt, "unit": "GN iter/s", "cores": ncores, "kind": "port",
                                      "ms_per_iter": dt * 1e3 / steps,
                                      "sample": "%d GN iterations of the same window, oracle/vio_oracle.c built with -fopenmp "
                                                "(landmark-parallel linearisation, Schur terms, back-substitution and chi2; "
                                                "the 171x171 LDLT stays serial), %d threads of the %d available" % (steps, ncores, navail)}
        except Exception as exc:      # a reported extra, never a reason to lose the line
            cpu_baseline_all_cores = {"error": str(exc)}

    # the reference's own backend (compiled from its sources where they lie, oracle/_ref, by the recipe in oracle/Makefile;
    # present when the repo was built where /root/reference exists): its dense (171+N)^2 solver needs 18 s and 13 GB per
    # iteration at N = 20 000, so it is timed on a 2 000-landmark window of the same generator and reported beside the port
    cpu_reference = None
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libvio_ref.so")
    if cpu_baseline is not None and os.path.exists(ref_so):
        try:
            rl = vio.VioLib(ref_so, "vior_")
            wr = make(2000, seed=42, obs_per_landmark=k_obs)
            cr = rl.context()
            cr.load(wr)
            cr.linearize()
            _, lam_r = cr.init_lm()
            cr.gn_iteration(lam_r)
            t = time.perf_counter()
            nref = 5
            for _ in range(nref):
                cr.gn_iteration(lam_r)
            dt = time.perf_counter() - t
            co2 = orc.context()
            co2.load(wr)
            co2.gn_iteration(lam_r)
            t = time.perf_counter()
            for _ in range(50):
                co2.gn_iteration(lam_r)
            dto = (time.perf_counter() - t) / 50
            cpu_reference = {"value": nref / dt, "unit": "GN iter/s", "cores": 1, "kind": "reference",
                             "ms_per_iter": dt * 1e3 / nref, "port_ms_per_iter_same_window": dto * 1e3,
                             "sample": "%d GN iterations of a 2000-landmark / %d-observation window (the reference's dense "
                                       "solver is O(N^2): 18 s per iteration at N = 20000, BASELINE.md section 2), "
                                       "oracle/_ref/libvio_ref.so, 1 thread" % (nref, wr.n_observations)}
        except Exception as exc:       # the reference library is optional test infrastructure
            cpu_reference = {"error": str(exc)}

    if rank == 0:
        lm_kind = "XYZ landmarks (VertexPointXYZ, 3x3 blocks)" if xyz else "inverse-depth landmarks"
        prior_txt = "no prior" if args.no_prior else "marginalisation prior of the preceding window"
        if world == 1:
            metric = "GN iterations/s, 11-frame (10-keyframe) window, 20k landmarks per GPU"
            workload = ("synthetic 11-frame VIO window (SURVEY.md 8d; BASELINE.json configs[2]): %d landmarks x %d observations, "
                        "10 IMU factors, %s, Cauchy loss, extrinsic fixed, fixed-lambda GN iteration, %s"
                        % (n_total, k_obs + (1 if xyz else 0), prior_txt, lm_kind))
            parallelism = "single GPU"
        else:
            metric = "GN iterations/s, 11-frame (10-keyframe) window, %dk landmarks sharded over the GPUs" % (n_total // 1000)
            workload = ("synthetic 11-frame VIO window (SURVEY.md 8d; BASELINE.json configs[3]): ONE window of %d landmarks x %d "
                        "observations, its landmarks block-sharded %d per GPU over %d GPUs (strong scaling: the window is the same "
                        "at every N > 1), 10 IMU factors and prior replicated, %s, Cauchy loss, extrinsic fixed, fixed-lambda GN "
                        "iteration, %s" % (n_total, k_obs + (1 if xyz else 0), n_per_gpu, world, prior_txt, lm_kind))
            parallelism = ("landmark-sharded x%d; per iteration one all-gather of the shards' 24 KB partial reduced systems, added in "
                           "rank order; the 171x171 pose solve replicated on every rank" % world)
        out = {
            "metric": metric,
            "value": value, "unit": "GN iter/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak" if world == 1 else "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": workload, "landmark_type": args.landmark_type,
                       "landmarks_per_gpu": n, "observations_per_gpu": m, "landmarks_total": n_total,
                       "lambda": lam, "parallelism": parallelism, "exchange": sb.exchange,
                       "rccl_ranks_seen": sb.ctx.comm_info()[0] if sb.exchange == "native" else 0,       # ncclCommCount of the library's communicator
                       "all_ranks_on_one_device": bool(one_device)},
            "final_chi2": chi2,
            "single_gpu_same_window_ms": single_gpu,
            "speedup_vs_single_gpu_same_window": (single_gpu / ms_per_step) if single_gpu else None,
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
            "replicas": replicas,
            "per_frame": per_frame,
            "per_frame_small": per_frame_small,
            "batched": batched,
            "scale_projection": scale_projection,
            "cpu_baseline_all_cores": cpu_baseline_all_cores,
            "cpu_reference": cpu_reference,
        }
        import ctypes
        ctypes.CDLL(None).fflush(None)      # RCCL's version banner sits in C stdio's buffer: keep the JSON line last
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        os.dup2(real_stdout_fd, 1)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
