#!/usr/bin/env python3
"""bench.py — frames/sec matched, 1080p frames vs a 500-page ORB set (BASELINE.json metric).

One "step" = one pass of the hot path (ORB detect+describe -> exact Hamming kNN
k=30 -> 5 % vote -> RANSAC similarity -> re-projection verdict) over one batch of
synthetic frames that is already resident in HBM when the timed region starts.
One process per GPU; ranks shard frames (weak scaling: the per-GPU batch is
fixed; --total-frames T: a fixed job, strong scaling), the page DB is replicated, and
each step ends with ONE RCCL all-gather of the per-frame verdict records, left on
the device by the library.  --workload cfg3: BASELINE configs[3] (the
216 000-frame lecture against a 1000-page deck: a fixed job, strong scaling, the page
timeline on rank 0); --workload cfg2: the SIFT + L2 matcher of configs[2] instead.

  python bench.py --gpus N --steps K --warmup W
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

Rank 0 prints one JSON line.  `roofline` is the dominant kernel (the exact
Hamming kNN: knn_tile2_kernel by default, knn_tile4_kernel with --knn mfma4, knn_hamming_kernel with --knn valu), timed with HIP events on its
launch stream inside the
library.  A plain run sets up, warms up, times the K steps and prints the line; --full adds what takes runs of its own
after the timed region: `cpu_baseline` (the CPU restatement, oracle/, kind "port", on a bounded sample of the same
workload on the host cores), `host_frames` (the PCIe-inclusive rate), the kernels with one batch in flight
(`roofline.one_batch_in_flight`, `stage_ms_one_batch_in_flight`) and, for cfg2, the in-run checks against the CPU
restatement and numpy.

--dump-outputs DIR writes the verdict records of the last timed step (every rank's, after the all-gather; cfg2:
rank 0's) as DIR/<field>.npy in float32 / float64: page_idx, similarity, inliers, n_keypoints.  The inputs are
seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # BASELINE.json metric: "frames/sec matched (1080p vs 500-page ORB set)"; SURVEY §8d "Headline"
    "headline": dict(frame=(1920, 1080), page=(2001, 1125), pages=500, nfeatures=1000, batch=256,
                     name="1080p frames vs 500-page deck, ORB-1000, exact Hamming kNN k=30 + 5% vote + RANSAC + reprojection verdict"),
    # BASELINE.json configs[1]
    "cfg1": dict(frame=(1920, 1080), page=(2001, 1125), pages=100, nfeatures=1000, batch=256,
                 name="configs[1]: 1080p batch=256 vs 100 pages, ORB-1000"),
    # BASELINE.json configs[3]: the 2 h 1080p@30fps lecture (216 000 frames) against a 1000-page deck, sharded over the GPUs, one
    # RCCL all-gather of the verdict records per step, the page timeline on rank 0.  A FIXED job (strong scaling): the K timed
    # steps process total_frames / (K x N) frames per GPU each, in units of `batch` frames drawn from a pool of `batch` distinct
    # synthetic frames per GPU that stays resident in HBM (the lecture's frames cycle through the pool; every unit runs the whole
    # hot path, nothing is cached).  ORB-1000 as in configs[1] (the config names no feature count).
    "cfg3": dict(frame=(1920, 1080), page=(2001, 1125), pages=1000, nfeatures=1000, batch=256, total_frames=216000, lecture=True,
                 name="configs[3]: 216 000-frame 1080p lecture vs 1000-page deck, ORB-1000, frames sharded over the GPUs, all-gather of verdicts, timeline on rank 0"),
    # BASELINE.json configs[4] shape on one GPU: 4K frames, ORB-2000, 1000-page deck (2 M train descriptors)
    # ("RANSAC homography verify": verify_model 1 = the 8-DOF model of include/slideo_amd.h on frames generated under a true
    # projective map; --verify-model 0 --persp 0 gives the reference's similarity model on similarity frames)
    "cfg4": dict(frame=(3840, 2160), page=(2001, 1125), pages=1000, nfeatures=2000, batch=64, verify_model=1, persp=0.1,
                 name="configs[4] shape: 4K frames batch=64 vs 1000 pages, ORB-2000, homography verification"),
    # BASELINE.json configs[2]: SIFT-128 descriptors, L2 BFMatcher as an N x M x 128 MFMA contraction, 1080p vs 500 pages:
    # SIFT on the device (csrc/sift.hip.h) feeding the int8 matrix-core L2 matcher (bench_cfg2).
    "cfg2": dict(frame=(1920, 1080), page=(2001, 1125), pages=500, nfeatures=1000, batch=256, knn_k=2,
                 name="configs[2]: SIFT-1000 detect + describe of 1080p frames, L2 k-NN (k=2, ratio-test shape) vs the SIFT descriptors of 500 pages"),
    # small, for smoke runs
    "tiny": dict(frame=(640, 360), page=(800, 450), pages=8, nfeatures=500, batch=16,
                 name="tiny: 640x360 vs 8 pages, ORB-500"),
}

# MI355X ceilings (MI355X_MICROARCH.md): 256 CU x 4 SIMD-32 x 2.4 GHz = 78.6e12 32-bit VALU lane-ops/s
# (= the 157.3 TFLOPS FP32 vector peak / 2); HBM3E 8 TB/s.
VALU_PEAK_TLANEOPS = 256 * 4 * 32 * 2.4e9 / 1e12
HBM_PEAK_GBS = 8000.0
MFMA_FP4_PEAK_TFLOPS = 10000.0   # dense FP4/FP6 MFMA peak (MI355X_MICROARCH.md; AMD's 20 PF figure is 2:1 sparse)
LANEOPS_PER_PAIR = 16          # 8 x v_xor_b32 + 8 x v_bcnt_u32_b32 per 256-bit pair


def host_cpu_budget():
    """CPUs this process may really use: logical CPUs, scheduler affinity, cgroup CPU quota (v2 cpu.max, v1 cfs_quota)."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    usable = aff if quota is None else max(1, min(aff, int(round(quota))))
    return {"logical": os.cpu_count() or 1, "affinity": aff, "cgroup_quota_cpus": quota, "usable": usable}


MFMA_I8_PEAK_TOPS = 5000.0       # dense int8 MFMA peak (2x the ~2.5 PF bf16 rate; the guide's microbenchmark reaches >= 3944)


def sift_like(rng, n):
    """OpenCV-SIFT-shaped descriptors: non-negative, most mass in few bins, L2 norm ~512, clipped to 255."""
    x = rng.gamma(0.6, 40.0, (n, 128)).astype(np.float32)
    x *= 512.0 / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-9)
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def bench_cfg2(args, wl, rank, world, local_rank, use_dist, barrier_fn):
    """configs[2] as a complete matcher (slideo_matcher_use_sift): per step one batch of 1080p frames, resident in HBM, through SIFT
    detect + describe (csrc/sift.hip.h), the squared-L2 2-NN of the 128-byte descriptors against the SIFT descriptors of the whole
    deck on the int8 matrix cores, Lowe's ratio test, and the path's own vote / RANSAC / rating / re-projection / verdict stages —
    page verdicts out, batches pipelined through the library's slots like the headline workload.  Checked inside the run, outside
    the timed region: the verdicts against the synthetic truth, frame 0's keypoints and descriptors against the CPU restatement of
    cv::SIFT (bit-exact), and 64 sampled queries' two nearest rows (public tap, same kernel) against numpy."""
    import torch
    import torch.distributed as dist
    from slideo_amd import _capi, synth
    B, P, nfeat, k = wl["batch"], wl["pages"], wl["nfeatures"], 2
    fw, fh = wl["frame"]; pw, ph = wl["page"]
    ratio = 0.75 if args.sift_vote == "ratio" else 0.0        # 0: the path's tolerance vote on the L2 distances (k = 30 rows)
    ncpu = os.cpu_count() or 1
    gen_threads = max(1, min(64, ncpu // max(world, 1)))
    t0 = time.time()
    pages = synth.pages(P, pw, ph, threads=gen_threads)
    frames, truth, _ = synth.frames(pages, B, fw, fh, first=rank * B, threads=gen_threads)
    t_gen = time.time() - t0
    m = _capi.Matcher(_capi.default_config(), device=local_rank)
    sc = _capi.sift_config(nfeatures=nfeat)
    m.use_sift(sc, ratio)
    t0 = time.time()
    for i in range(0, P, 50):
        m.add_pages(list(pages[i:i + 50]))
    m.finalize()
    torch.cuda.synchronize()
    t_db = time.time() - t0
    nt = m.descriptor_count
    d_frames = torch.from_numpy(frames).cuda()               # inputs resident in HBM before timing
    depth = max(1, min(args.inflight or m.max_in_flight(), m.max_in_flight()))

    def run_steps(n):
        pending, v = [], None
        for _ in range(n):
            if len(pending) == depth:
                v = m.collect(pending.pop(0))
            pending.append(m.submit_dev(d_frames.data_ptr(), B, fw, fh))
        while pending:
            v = m.collect(pending.pop(0))
        return v

    if args.warmup:
        run_steps(args.warmup)
    m.set_profiling(True)
    barrier_fn()
    t0 = time.perf_counter()
    v = run_steps(args.steps)
    barrier_fn()
    dt = time.perf_counter() - t0
    if use_dist:
        td = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(td, op=dist.ReduceOp.MAX)
        dt = float(td.item())
    prof, _ = m.read_profile()
    m.set_profiling(False)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, v)
    # ---- checkers (outside the timed region; --full)
    acc = float((v["page_idx"] == truth).mean())
    nq = int(v["n_keypoints"].sum())
    knn_ok = sift_ok = None
    if args.full:
        gk0, gd0 = m.sift(frames[0], sc)
        assert len(gk0) == int(v["n_keypoints"][0]), "the matcher's frame 0 has another keypoint count than the SIFT tap"
        t_rows = np.concatenate([m.page_features(p_)[1] for p_ in range(0, P, max(1, P // 40))][:40])      # a sample of the deck's rows
        sample = np.random.default_rng(5).integers(0, len(gd0), 64)
        gi, gdist = m.knn_l2_u8(gd0[sample], t_rows, 2)
        knn_ok = True
        for j, i in enumerate(sample):
            diff = t_rows.astype(np.int32) - gd0[i].astype(np.int32)
            d2 = (diff * diff).sum(1)
            order = np.lexsort((np.arange(len(t_rows)), d2))[:2]
            knn_ok &= bool(np.array_equal(order, gi[j]) and np.array_equal(d2[order].astype(np.uint32), gdist[j]))
        assert knn_ok, "L2 k-NN disagrees with the numpy recomputation"
    if args.full and rank == 0 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import pyoracle
        t1 = time.time()
        ok_, od_, _ = pyoracle.sift(frames[0], pyoracle.sift_config(nfeatures=nfeat))
        t_cpu1 = time.time() - t1
        sift_ok = bool(len(ok_) == len(gk0) and np.array_equal(od_, gd0) and np.array_equal(ok_["x"], gk0["x"]) and np.array_equal(ok_["angle"], gk0["angle"]))
        assert sift_ok, "SIFT of frame 0 differs from the CPU restatement"
    ms = 1e3 * dt / args.steps
    s_avg = prof["orb"][0] / max(prof["orb"][1], 1)          # stage 0 of the unit = the extractor (SIFT here)
    k_avg = prof["knn"][0] / max(prof["knn"][1], 1)          # stage 1 = the L2 search + the ratio-test lists
    v_avg = prof["verify"][0] / max(prof["verify"][1], 1)
    pairs = float(nq) * nt
    # SIFT stage traffic model (csrc/sift.hip.h header): per frame the doubled base image (4 w h floats) is written once, and per
    # octave 5 blurred layers + 5 DoG layers are written and 5 layers read: (1 + 15 x 4/3) x 16 w h bytes
    sift_bytes = (1 + 15 * 4.0 / 3.0) * 16.0 * fw * fh
    out = {
        "metric": "frames/sec matched (SIFT-128 + L2 k-NN + ratio test + RANSAC + reprojection verdict, 1080p vs 500 pages)",
        "value": round(B * world * args.steps / dt, 2), "unit": "frames/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32 (SIFT) + i8 (L2 k-NN)", "data": "synthetic",
        "config": {"workload": wl["name"], "frame": [fw, fh], "page": [pw, ph], "pages": P, "sift_nfeatures": nfeat, "train_descriptors_M": int(nt),
                   "frames_per_step_per_gpu": B, "query_descriptors_per_step": int(nq), "mean_keypoints_per_frame": round(nq / B, 1),
                   "knn": ("exact brute force squared L2, k=2, v_mfma_i32_32x32x32_i8; Lowe's ratio test %.2f" % ratio) if ratio > 0 else
                          "exact brute force squared L2, k=30, v_mfma_i32_32x32x32_i8; the path's 5 % tolerance vote on the L2 distances",
                   "sift_vote": args.sift_vote,
                   "stages": "slideo_matcher_use_sift: SIFT detect + describe -> L2 2-NN against the deck's SIFT descriptors -> ratio test -> "
                             "per-page vote -> RANSAC similarity -> rating -> re-projection -> verdict; the reference has no SIFT / float-descriptor "
                             "path (SURVEY F6)",
                   "parallelism": "frames sharded over %d GPU(s), page DB replicated; %d batches in flight per GPU (the extraction stages take "
                                  "turns on the matcher's SIFT workspace, the verify stages overlap them)" % (world, depth),
                   "page_db_build_s": round(t_db, 2), "input_gen_s": round(t_gen, 2),
                   "accuracy_vs_synthetic_truth": round(acc, 4),
                   "checked": {"knn_vs_numpy_64_queries": knn_ok, "sift_frame0_bit_exact_vs_cpu_restatement": sift_ok}},
        "roofline": {"kernel": "knn_l2_kernel", "bound": "mfma", "achieved": round(pairs * 256 / (k_avg * 1e-3) / 1e12, 2),
                     "peak": MFMA_I8_PEAK_TOPS, "unit": "TFLOP/s", "frac": round(pairs * 256 / (k_avg * 1e-3) / 1e12 / MFMA_I8_PEAK_TOPS, 4),
                     "flops_per_pair": 256, "traffic": None, "avg_launch_ms": round(k_avg, 4), "launches": int(prof["knn"][1]),
                     "pairs_per_launch": int(pairs), "interval": "knn_l2_kernel + unpack + ratio-test lists, HIP events on the launch stream"},
        "sift_stage": {"bound": "hbm", "avg_ms_per_batch": round(s_avg, 3), "algorithmic_bytes_per_frame": int(sift_bytes),
                       "achieved": round(sift_bytes * B / (s_avg * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": round(sift_bytes * B / (s_avg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                       "interval": "all kernels of the unit's SIFT stage for one batch, HIP events on the launch stream"},
        "stage_ms_per_batch": {"sift": round(s_avg, 3), "l2_knn": round(k_avg, 3), "verify": round(v_avg, 3)},
    }
    if sift_ok is not None:
        out["cpu_baseline"] = {"value": round(1.0 / t_cpu1, 3), "unit": "frames/s", "cores": 1, "kind": "port",
                               "sample": "SIFT of frame 0 on one core (oracle/sift_oracle.h), %.2f s; the L2 k-NN and verify stages are not in it" % t_cpu1}
    if rank == 0:
        print(json.dumps(out), flush=True)
    m.close()


def dump_outputs(dirname, recs):
    """--dump-outputs: the verdict records a caller of the timed path receives, one .npy per field (float64 holds the int32
    fields exactly, similarity stays float32)."""
    os.makedirs(dirname, exist_ok=True)
    for name in recs.dtype.names:
        col = recs[name]
        np.save(os.path.join(dirname, name + ".npy"), col.astype(np.float32 if col.dtype == np.float32 else np.float64))


def knn_kernel_label(args):
    """The search kernel(s) a run launches (stage_knn.hip knn_shape / SLIDEO_KNN_SHARE; --knn mfma4 = the 4-tile A/B shape)."""
    if args.knn == "mfma4":
        return "knn_tile4_kernel"
    share = os.environ.get("SLIDEO_KNN_SHARE", "auto")
    t1 = "knn_tile1w12_kernel (12 waves x 1 query tile, 88 registers: measurement mode)"
    t2 = "knn_tile2_kernel (8 waves x 2 query tiles)"
    w12 = "knn_tile2w12_kernel (12 waves x 2 query tiles)"
    auto = t2 + ": one block per CU while units share the chip, two otherwise; " + w12 + " instead while units share the chip from SLIDEO_KNN_W12_RATIO (290) pairs per frame pixel on"
    return {"auto": auto, "-1": auto, "5": t1 + " while units share the chip, else " + t2, "6": t1, "0": t2 + ", two blocks per CU",
            "1": t2 + ", one block per CU", "3": w12 + " while units share the chip, else " + t2, "4": w12}.get(share, t2)


def self_launch(n):
    """Re-executes this command line under torch.distributed.run with n ranks on this node; returns its exit code."""
    import socket
    import subprocess
    with socket.socket() as so:                      # a free rendezvous port on the loopback interface
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="headline", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="frames per step per GPU (default: workload's)")
    ap.add_argument("--pages", type=int, default=0)
    ap.add_argument("--knn", default="mfma", choices=["mfma", "mfma2", "mfma4", "valu"], help="kNN engine (identical results)")
    ap.add_argument("--no-overlap", action="store_true", help="one batch in flight (for per-kernel profiling)")
    ap.add_argument("--inflight", type=int, default=0, help="batches in flight (default and maximum: the library's slots)")
    ap.add_argument("--total-frames", type=int, default=0,
                    help="strong scaling: the job is this many frames in all (BASELINE configs[3] is a fixed 216 000-frame job); each of the "
                         "K timed steps then processes total/(K*N) frames per GPU instead of the workload's fixed per-GPU batch")
    ap.add_argument("--verify-model", type=int, default=-1, choices=[-1, 0, 1],
                    help="geometric model of the verification: 0 = the reference's 4-DOF similarity (estimateAffinePartial2D), 1 = 8-DOF homography "
                         "(findHomography + warpPerspective; default: the workload's, 1 for cfg4, else 0)")
    ap.add_argument("--hdlt", type=int, default=-1, choices=[-1, 0, 1, 2],
                    help="verify_model 1: how a 4-point sample becomes a model (slideo_ocv_variants.hdlt): 0 = cv::findHomography's L^T L + Jacobi eigenvectors "
                         "(the fidelity switch), 1 = the 8x8 system by Gaussian elimination (same models to f64 round-off, ~60x cheaper per sample; "
                         "the LIBRARY'S DEFAULT since ABI 6 — end-to-end agreement with form 0 measured in profiles/r04_hdlt_agreement.json), 2 = the closed form "
                         "(square-to-quad maps); default: the library's")
    ap.add_argument("--verdict-rule", type=int, default=0, choices=[0, 1],
                    help="0 = the reference's verdict (best re-projection similarity wins, mo/lib.rs:370-389); 1 = the opt-in departure "
                         "slideo_config.verdict_rule: rating order, similarity only accepts")
    ap.add_argument("--pool", type=int, default=0, help="distinct resident frames per GPU the stream of frames cycles through (default: the workload's batch)")
    ap.add_argument("--unit", type=int, default=0, help="frames per submitted unit (default: the pool, i.e. one unit per step in weak mode)")
    ap.add_argument("--matcher", default="exact", choices=["exact", "lsh"],
                    help="descriptor index: exact brute force (default; north_star) or the LSH candidate rule of the reference's FLANN index "
                         "(slideo_config.matcher 1: 6 tables, 12-bit keys, multi-probe 1 — recall < 1, and on these descriptors SLOWER than the exact "
                         "matrix-core search: the skewed buckets make a fifth of all rows candidates of a query)")
    ap.add_argument("--sift-vote", choices=["ratio", "tolerance"], default="tolerance",
                    help="cfg2 (SIFT matcher mode): who votes — the path's own 5 %% tolerance vote on the 30 nearest rows (default: it keeps the "
                         "matches between pages of one template, accuracy 1.00 on the synthetic decks), or Lowe's ratio test on the two nearest "
                         "rows (the north_star's wording; drops exactly those matches: accuracy 0.71)")
    ap.add_argument("--persp", type=float, default=-1.0, help="projective component of the synthetic frames (0 = similarity frames; default: the workload's)")
    ap.add_argument("--backend", default="", choices=["", "nccl", "gloo"],
                    help="collective backend (default: SLIDEO_BENCH_BACKEND or nccl = RCCL). gloo: the verdict all-gather goes through host "
                         "memory — a control-flow dry run of the N-rank job on a box with fewer GPUs than ranks (with --share-device)")
    ap.add_argument("--share-device", action="store_true",
                    help="gloo only: ranks may share devices (rank r uses device r mod the visible GPUs). Never a measurement of scaling.")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what takes runs of its own after the timed region: the CPU baseline, the host-frames "
                         "record, the kernels with one batch in flight, cfg2's checks against the CPU restatement and numpy")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write the verdict records of the last timed step as DIR/<field>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-host-frames", action="store_true", help="--full without the PCIe-inclusive host-frames record (3 calls after the timed region)")
    ap.add_argument("--cpu-sample", type=int, default=0, help="frames in the CPU baseline sample")
    args = ap.parse_args()

    # (Hardware queues: an initialised RCCL communicator has created streams before the matcher's; with the HIP runtime's default
    # of four hardware queues two of the matcher's slot streams used to land on ONE queue and every rank of a multi-GPU run was 10 %
    # slower than the single-GPU run — profiles/r06_experiments.txt 6.  The library now picks its slot streams by measurement
    # (slideo_matcher_create, SLIDEO_STREAM_PICK), so nothing is set here; config.gpu_max_hw_queues records what the process ran with.)
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or os.environ.get("SLIDEO_BENCH_FORCE_LAUNCH") == "1"):
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU, rendezvous on 127.0.0.1) and
        # hand their output through — the same command line the driver's torch.distributed.run form runs
        sys.exit(self_launch(args.gpus))
    if world != args.gpus:
        args.gpus = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback) [rank %d of %d]" % (rank, world))
    # SLIDEO_BENCH_BACKEND=gloo lets the N>1 control flow be exercised on a box with fewer GPUs than ranks (ranks then
    # share devices and the verdict all-gather goes through host memory); the driver's runs use nccl = RCCL.
    backend = args.backend or os.environ.get("SLIDEO_BENCH_BACKEND", "nccl")
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if args.share_device and backend == "nccl":
        raise SystemExit("bench.py: --share-device needs --backend gloo (RCCL needs one GPU per rank)")
    if backend == "nccl" and torch.cuda.device_count() < local_world:
        # RCCL needs one device per rank; two ranks on one device do not fail, they hang in the first collective
        raise SystemExit("bench.py: %d ranks on this node but %d GPU(s) visible — the nccl (= RCCL) backend needs one GPU per rank "
                         "[rank %d of %d]; SLIDEO_BENCH_BACKEND=gloo lets ranks share devices (control-flow tests only)"
                         % (local_world, torch.cuda.device_count(), rank, world))
    if backend != "nccl":
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    # SLIDEO_BENCH_FORCE_DIST=1: run the process-group set-up and the per-step all-gather at world size 1 too (under torchrun
    # --nproc-per-node 1), so that the RCCL code path executes on a single-GPU box (tests/test_bench_contract.py)
    use_dist = world > 1 or (os.environ.get("SLIDEO_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    from slideo_amd import _capi, synth

    wl = dict(WORKLOADS[args.workload])
    if args.batch: wl["batch"] = args.batch
    if args.pages: wl["pages"] = args.pages
    if args.workload == "cfg2":
        def _barrier():
            if use_dist:
                dist.barrier()
            torch.cuda.synchronize()
        bench_cfg2(args, wl, rank, world, local_rank, use_dist, _barrier)
        if use_dist:
            dist.destroy_process_group()
        return
    fw, fh = wl["frame"]; pw, ph = wl["page"]
    B, P = wl["batch"], wl["pages"]
    if not args.total_frames:
        args.total_frames = wl.get("total_frames", 0)
    strong = args.total_frames > 0
    if strong:                                   # fixed total job: per-GPU frames per step shrink as GPUs are added
        B = max(1, args.total_frames // (max(args.steps, 1) * world))
    # A step's B frames go through the library in UNITS of at most `pool` frames, drawn from a pool of `pool` distinct frames per
    # GPU that is resident in HBM before the timed region (weak mode and the small strong-mode jobs: pool = B, one unit per step,
    # as before; configs[3]: 10 800 frames per step at N = 1 cycle through 256 resident ones — every unit runs the whole hot path).
    # The frames of the timed region form ONE stream, frame g = resident frame g mod `pool` (pool distinct frames per GPU, in HBM
    # before the timed region), cut into UNITS of U frames that go through the library's slots; a step is the B frames [sB, (s+1)B) of
    # that stream, whatever units they travel in, and its verdict records are gathered once all of them are in.  Weak mode by default:
    # pool = B = U, one unit per step.  configs[3]: 10 800 frames per step at N = 1 cycle through 256 resident ones, 43 units per step.
    # --unit U: another unit size over the same stream (measured r05: 176 / 192 / 200 / 256-frame units give the same rate within 0.5 %).
    pool = min(B, args.pool or wl["batch"])
    U = max(1, min(args.unit or wl.get("unit", 0) or pool, pool))
    units_per_step = B / U
    ncpu = os.cpu_count() or 1
    gen_threads = max(1, min(64, ncpu // max(world, 1)))

    # ---- synthetic inputs (seeded; same pages on every rank, disjoint frame ranges per rank)
    t0 = time.time()
    pages = synth.pages(P, pw, ph, threads=gen_threads)
    verify_model = wl.get("verify_model", 0) if args.verify_model < 0 else args.verify_model
    persp = wl.get("persp", 0.0) if args.persp < 0 else args.persp
    if args.hdlt < 0:
        args.hdlt = _capi.default_config().ocv.hdlt          # the library's default (1 since ABI 6)
    if persp > 0:
        frames, truth, _ = synth.frames_persp(pages, pool, fw, fh, persp=persp, first=rank * pool, threads=gen_threads)
    else:
        frames, truth, _ = synth.frames(pages, pool, fw, fh, first=rank * pool, threads=gen_threads)
    truth_of = lambda g0, n: truth[(g0 + np.arange(n)) % pool]            # the truth of stream frames g0 .. g0 + n - 1
    t_gen = time.time() - t0

    cfg = _capi.default_config(nfeatures=wl["nfeatures"], verify_model=verify_model, ocv_hdlt=args.hdlt, matcher=1 if args.matcher == "lsh" else 0,
                               verdict_rule=args.verdict_rule)
    m = _capi.Matcher(cfg, device=local_rank)
    m.set_knn_engine(args.knn)
    args.inflight = min(args.inflight or m.max_in_flight(), m.max_in_flight())
    t0 = time.time()
    CH = 50
    for i in range(0, P, CH):
        m.add_pages(list(pages[i:i + CH]))
    m.finalize()
    torch.cuda.synchronize()
    t_db = time.time() - t0
    M = m.descriptor_count
    Mu = m.unique_descriptor_count             # what the k-NN stage searches (equal rows collapsed, results unchanged)

    # (a unit's frames must be contiguous in memory: when U does not divide the pool, the pool's first U frames are repeated behind it)
    d_frames = torch.from_numpy(frames if pool % U == 0 else np.concatenate([frames, frames[:U]])).cuda()     # inputs resident in HBM before timing
    frame_bytes = fh * fw * 3
    stream = torch.cuda.current_stream().cuda_stream
    verdict_words = 4
    coll_dev = "cuda" if backend == "nccl" else "cpu"
    # The library leaves a unit's verdict records in a RING of R records in device memory, at the unit's place in the stream (R a
    # multiple of U and of B: neither a unit nor a step wraps); the step's all-gather reads its B records on torch's stream, and an
    # event recorded behind the collective guards the region's NEXT use, R / B steps later — by then it has long completed, so no
    # step ends in a host wait for the collective.
    lcm = U * B // int(np.gcd(U, B))
    R = lcm * max(1, -(-((args.inflight + 3) * max(U, B)) // lcm))
    ring = torch.zeros((R, verdict_words), dtype=torch.int32, device=coll_dev)
    ring_host = np.zeros(R, _capi.VERDICT_DTYPE)
    step_done_ev = [None] * (R // B)
    d_all = torch.zeros((world * B, verdict_words), dtype=torch.int32, device=coll_dev) if use_dist else None
    on_dev = use_dist and coll_dev == "cuda"          # the library leaves the records on the device
    st = {"next_step": 0, "last": None}
    host_t = {"event_wait": 0.0, "collect": 0.0, "all_gather": 0.0, "submit": 0.0}     # host seconds of the stream loop's calls (cleared before the timed region)

    def collect_unit(item, local):
        """Collects one unit into its place in the ring; behind the LAST unit of a step — unless `local` — the step's one collective
        (RCCL over xGMI) runs on the step's verdict records."""
        ticket, g0, n = item
        gather = use_dist and not local and os.environ.get("SLIDEO_BENCH_SKIP_GATHER") != "1"      # (the switch: measurement only — where a collective path's time goes)
        r0 = g0 % R
        tq0 = time.perf_counter()
        if gather and on_dev:
            for sl in range(r0 // B, (r0 + n - 1) // B + 1):
                if step_done_ev[sl] is not None:
                    step_done_ev[sl].synchronize()   # an event R / B steps old: returns at once
        tq1 = time.perf_counter()
        v = m.collect(ticket, dev_out=(ring.data_ptr() + r0 * 4 * verdict_words) if (gather and on_dev) else 0)
        tq2 = time.perf_counter()
        host_t["event_wait"] += tq1 - tq0; host_t["collect"] += tq2 - tq1
        ring_host[r0:r0 + n] = v
        if gather and not on_dev:                    # gloo stand-in: host tensors
            ring[r0:r0 + n].copy_(torch.from_numpy(v.view(np.int32).reshape(n, verdict_words)), non_blocking=False)
        while (st["next_step"] + 1) * B <= g0 + n:   # units are collected in order: every frame before g0 + n is in
            a = (st["next_step"] * B) % R
            st["last"] = (st["next_step"], ring_host[a:a + B].copy())
            if gather:
                tq3 = time.perf_counter()
                dist.all_gather_into_tensor(d_all, ring[a:a + B])      # the one collective of the path
                if on_dev:
                    step_done_ev[a // B] = torch.cuda.Event()
                    step_done_ev[a // B].record()
                host_t["all_gather"] += time.perf_counter() - tq3
            st["next_step"] += 1

    def run_stream(total, depth=None, local=False, first_unit_only=False):
        """`total` frames of the stream, in units of U frames (the last one may be shorter).  `depth` units are kept in flight (submit
        i+depth-1 before collecting i) so that the ORB / verify stages of some units share the GPU with the kNN of others.
        Returns (verdicts of the last complete step or None, that step's first frame's place in the stream)."""
        pending = []
        depth = depth or (1 if args.no_overlap else max(1, args.inflight))
        st["next_step"], st["last"] = 0, None
        g = 0
        while g < total:
            n = min(U, total - g)
            g_read = 0 if first_unit_only else g        # (profiling the kernels alone: the same first unit every time)
            if len(pending) == depth:
                collect_unit(pending.pop(0), local)
            tq4 = time.perf_counter()
            pending.append((m.submit_dev(d_frames.data_ptr() + (g_read % pool) * frame_bytes, n, fw, fh, stream=stream), g, n))
            host_t["submit"] += time.perf_counter() - tq4
            g += n
        while pending:
            collect_unit(pending.pop(0), local)
        return (st["last"][1], st["last"][0] * B) if st["last"] else (None, 0)

    def run_steps(k):
        """k steps = the k * B first frames of the stream"""
        return run_stream(k * B)

    def barrier():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    if args.warmup:
        run_steps(args.warmup)
    m.set_profiling(True)
    barrier()
    for k_ in host_t: host_t[k_] = 0.0
    t0 = time.perf_counter()
    v, g_last = run_steps(args.steps)
    barrier()
    dt = time.perf_counter() - t0
    host_ms = {k_: round(v_ / max(args.steps, 1) * 1e3, 4) for k_, v_ in host_t.items()}
    prof, knn_pairs = m.read_profile()
    clk_mhz, clk_n = m.read_shader_clock()          # (the search blocks of the timed region; cleared by the read)
    m.set_profiling(False)
    # outside the timed region: the same launches with one batch in flight, i.e. each kernel alone on the GPU
    # (under overlap the kNN shares the CUs with the other batch's ORB / verify kernels and its launches stretch)
    prof_alone = None
    if args.full and rank == 0 and not args.no_overlap and args.inflight > 1:
        m.set_profiling(True)
        run_stream(3 * U, depth=1, local=True, first_unit_only=True)      # (three launches of the stream's first unit)
        torch.cuda.synchronize()
        prof_alone, pairs_alone = m.read_profile()
        m.set_profiling(False)
    gathered_ok = True
    if use_dist:
        tmax = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        # the gathered records of the last step: this rank's slice must be its own verdicts
        mine = d_all[rank * B:(rank + 1) * B].cpu().numpy().view(_capi.VERDICT_DTYPE).reshape(-1)
        gathered_ok = bool(np.array_equal(mine, v))
    if args.dump_outputs and rank == 0:
        gathered = use_dist and os.environ.get("SLIDEO_BENCH_SKIP_GATHER") != "1"
        dump_outputs(args.dump_outputs, d_all.cpu().numpy().view(_capi.VERDICT_DTYPE).reshape(-1) if gathered else v)

    truth_step = truth_of(g_last, B)                # the truth of the last step's frames
    acc = float((v["page_idx"] == truth_step).mean())
    total_frames = args.steps * B * world
    fps = total_frames / dt

    # configs[3]: the page timeline on rank 0 from the gathered records of the last step — the end-of-video sentinel, the sort by
    # time and the removal of consecutive duplicates of mo/lib.rs:185-189,229-244 (slideo_amd/distributed.py timeline) over this
    # step's share of the lecture (its world x B sampled frames, 5 s apart: mo/lib.rs:145,175), beside the same over the truth
    lecture = None
    if wl.get("lecture"):
        from slideo_amd import distributed as D
        if use_dist:
            t_all = torch.zeros(world * B, dtype=torch.int32, device=coll_dev)
            dist.all_gather_into_tensor(t_all, torch.from_numpy(truth_step.astype(np.int32)).to(coll_dev))
            truth_all = t_all.cpu().numpy()
            v_all = d_all.cpu().numpy().view(_capi.VERDICT_DTYPE).reshape(-1)
        else:
            truth_all, v_all = truth_step, v
        if rank == 0:
            S = len(v_all)
            times = 5.0 * np.arange(S)
            fidx = (times * 30.0).astype(np.int64)
            tl = D.timeline(v_all, times, fidx, 5.0 * S, int(5.0 * S * 30.0))
            tv = np.zeros(S, _capi.VERDICT_DTYPE); tv["page_idx"] = truth_all
            tt = D.timeline(tv, times, fidx, 5.0 * S, int(5.0 * S * 30.0))
            lecture = {"sampled_frames_in_the_last_step": S, "timeline_entries": len(tl), "truth_entries": len(tt),
                       "entries_equal_to_truth": len(set(tl) & set(tt)),
                       "job": "%d frames = %d steps x %d GPU(s) x %d frames; a GPU's frames run as units of %d frames (%.2f units per step)"
                              % (total_frames, args.steps, world, B, U, units_per_step)}

    out = {
        "metric": "frames/sec matched (1080p vs 500-page ORB set)" if args.workload == "headline" else "frames/sec matched",
        "value": round(fps, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "strong" if strong else "weak",
        "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": wl["name"], "frame": [fw, fh], "page": [pw, ph], "pages": P, "nfeatures": wl["nfeatures"],
                   "train_descriptors_M": int(M), "train_descriptors_unique": int(Mu), "frames_per_step_per_gpu": B,
                   "knn": ("exact brute force, k=30, engine=%s; overlapped batches launch the search with one block per CU (SLIDEO_KNN_SHARE=%s)" % (args.knn, os.environ.get("SLIDEO_KNN_SHARE", "auto"))) if args.matcher == "exact" else "LSH candidates (6 tables x 12 bits, multi-probe 1), k=30 nearest candidates",
                   "verify_model": verify_model, "ocv_hdlt": args.hdlt, "verify": ("8-DOF homography: findHomography(RANSAC) + warpPerspective" if verify_model == 1 else "the reference's 4-DOF similarity: estimateAffinePartial2D + warpAffine"),
                   "frames_projective_component": persp,
                   "parallelism": "frames sharded over %d GPU(s), page DB replicated, 1 RCCL all-gather of verdicts per step (device to device); %d batches in flight per GPU, one HIP stream each" % (world, 1 if args.no_overlap else args.inflight),
                   "inputs": "%d distinct synthetic frames per GPU, resident in HBM before the timed region; the timed region's %d frames per GPU are ONE stream (frame g = resident frame g mod %d) submitted in units of %d frames, a step = %d consecutive frames of it; every unit runs the whole hot path (the PCIe-inclusive rate with host frames is in DESIGN.md section 6)" % (pool, args.steps * B, pool, U, B),
                   "frames_per_unit": U, "units_per_step": round(units_per_step, 3),
                   "search_pairs_per_frame_pixel": round(float(wl["nfeatures"]) * float(Mu) / float(fw * fh), 1), "resident_pool_frames_per_gpu": pool, "lecture": lecture,
                   "collective": ({"backend": backend, "all_gather_of_verdicts_checked": gathered_ok} if use_dist else None),
                   "host_ms_per_step": host_ms, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "default (4)"),
                   "page_db_build_s": round(t_db, 2), "input_gen_s": round(t_gen, 2),
                   "accuracy_vs_synthetic_truth": round(acc, 4),
                   "mean_keypoints_per_frame": round(float(v["n_keypoints"].mean()), 1)},
    }
    if rank == 0:
        knn_ms, knn_n = prof["knn"]
        if knn_n > 0:
            avg_s = knn_ms / knn_n * 1e-3
            pairs_per_launch = knn_pairs / knn_n
            # (pairs = query descriptors x train rows EVALUATED: the matrix-core engine searches the Mu distinct rows of the M train
            # descriptors and restores the full-set result exactly — knn_expand_dups_kernel, inside the timed interval)
            Mk = Mu if args.knn != "valu" else M
            q_per_launch = pairs_per_launch / max(Mk, 1)
            # minimal operand traffic: packed queries + packed train once, 32 keys per query out
            alg_bytes = 32.0 * (q_per_launch + Mk) + q_per_launch * 32 * 4
            hbm_view = {"bound": "hbm", "achieved": round(alg_bytes / avg_s / 1e9, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(alg_bytes / avg_s / 1e9 / HBM_PEAK_GBS, 6), "algorithmic_bytes_per_launch": int(alg_bytes)}
            # HBM-side bytes per launch from rocprofv3 PMC passes (profiles/knn_traffic.json; FETCH_SIZE doubled
            # per the gfx950 correction).  Measured offline on this exact workload; null for any other.
            traffic = None
            if args.workload == "headline" and args.knn == "mfma" and not args.batch and not args.pages:
                try:
                    here = os.path.dirname(os.path.abspath(__file__))
                    tj = json.load(open(os.path.join(here, "profiles", "knn_traffic.json")))
                    # the figure was measured offline on ONE build of the kernel over ONE train matrix: it is only reported while the
                    # kernel source and the matrix size are the ones it was measured on (otherwise null — never a stale number)
                    import hashlib
                    sha = hashlib.sha1(open(os.path.join(here, "slideo_amd", "csrc", "knn_tile.hip.h"), "rb").read()).hexdigest()
                    if tj.get("kernel_source_sha1") == sha and int(tj.get("train_rows_searched", -1)) == int(Mk):
                        fx2, wr, nd = 2 * tj["fetch_size_kib"], tj["write_size_kib"], tj["dispatches"]
                        traffic = {"bytes_per_launch": int((fx2 + wr) / nd * 1024), "fetch_kib_x2": int(fx2 / nd), "write_kib": int(wr / nd),
                                   "source": tj["source"], "note": tj["note"]}
                    else:
                        traffic = None
                except (OSError, KeyError, ValueError):
                    traffic = None
            # `traffic` = HBM bytes per launch (a number, or null where it was not measured); the passes behind it in traffic_detail
            # ---- the roofline record.  TOP LEVEL = anchored on the driver's clock: the matrix-pipe flops a step's
            # launches EXECUTE over ms_per_step, so that  frac x peak x ms_per_step == flops_per_step  by construction and the kernel's
            # time per step cannot exceed the step.  The per-launch figure (a launch's flops over its own HIP-event duration inside the
            # timed region) is an OCCUPANCY statement since round 4 — overlapped units launch the search one block per CU beside the
            # other stages and consecutive launches overlap each other, so a launch lasts longer than a step and its rate falls when
            # the job gets faster: it lives in `per_launch`.  The kernel with the chip to itself is `one_batch_in_flight`.
            step_s = out["ms_per_step"] * 1e-3
            launches_per_step = knn_n / max(args.steps, 1)
            common = {"traffic": traffic["bytes_per_launch"] if traffic else None, "traffic_detail": traffic,
                      "launches_per_step": round(launches_per_step, 3), "pairs_per_launch": int(pairs_per_launch),
                      "interval": "ms_per_step (barrier + synchronize on both sides of the timed steps): what a step's launches execute / the step",
                      "shader_clock_mhz": (round(clk_mhz, 1) if clk_n else None),
                      "shader_clock_note": "s_memtime / s_memrealtime deltas summed over the search blocks of the timed region (every 8th block records; %d samples): the clock the search waves ran at" % clk_n,
                      "hbm_view": hbm_view}
            per_launch_note = ("a launch's own duration (search kernel + its list merge, HIP events on the launch stream) inside the timed region. With several "
                               "units in flight a launch shares every CU with the ORB / verify kernels of the other units and overlaps the next unit's "
                               "launch: an occupancy figure (launches_per_step x avg_launch_ms may exceed ms_per_step), not the kernel's rate")
            if args.knn != "valu":
                # Hamming = |q| + |t| - 2 <q, t> on {0,1} FP4 operands: 2 * 256 flops per pair.  Executed pairs = query
                # descriptors x DISTINCT train rows (K x Mu; equal rows are collapsed at finalize and restored in the lists by
                # knn_expand_dups_kernel); SURVEY 8(d)'s K x M count over ALL rows is `algorithmic` (effective, not executed).
                flops_launch = 2.0 * 256 * pairs_per_launch
                flops_step = flops_launch * launches_per_step
                achieved = flops_step / step_s / 1e12
                alg_step = 2.0 * 256 * (q_per_launch * M) * launches_per_step / step_s / 1e12
                assert achieved <= MFMA_FP4_PEAK_TFLOPS, "executed matrix-core rate above the peak: the pair count or the timing is wrong"
                out["roofline"] = dict({"kernel": "%s (v_mfma_f32_32x32x64_f8f6f4, {0,1} FP4 x FP4)" % knn_kernel_label(args), "bound": "mfma",
                                        "achieved": round(achieved, 4), "peak": MFMA_FP4_PEAK_TFLOPS, "unit": "TFLOP/s",
                                        "frac": round(achieved / MFMA_FP4_PEAK_TFLOPS, 7), "flops_per_pair": 512, "flops_per_step": flops_step,
                                        "counts": "executed pairs: query descriptors x DISTINCT train rows (K x Mu)",
                                        "algorithmic": {"pairs_per_launch": int(q_per_launch * M), "achieved": round(alg_step, 4), "frac": round(alg_step / MFMA_FP4_PEAK_TFLOPS, 7),
                                                        "note": "SURVEY 8(d)'s definition, K x M pairs over ALL train rows x 512 flops over the same step: the rate a search "
                                                                "without the train-set de-duplication would need (effective, not executed)"},
                                        "per_launch": {"avg_launch_ms": round(avg_s * 1e3, 4), "launches": int(knn_n), "achieved": round(flops_launch / avg_s / 1e12, 2),
                                                       "frac": round(flops_launch / avg_s / 1e12 / MFMA_FP4_PEAK_TFLOPS, 4), "note": per_launch_note}}, **common)
            else:
                laneops_launch = LANEOPS_PER_PAIR * pairs_per_launch
                achieved = laneops_launch * launches_per_step / step_s / 1e12
                out["roofline"] = dict({"kernel": "knn_hamming_kernel<32> (v_xor_b32 + v_bcnt_u32_b32)", "bound": "valu",
                                        "achieved": round(achieved, 5), "peak": round(VALU_PEAK_TLANEOPS, 2), "unit": "Tlaneop/s",
                                        "frac": round(achieved / VALU_PEAK_TLANEOPS, 7), "laneops_per_pair": LANEOPS_PER_PAIR,
                                        "flops_per_step": laneops_launch * launches_per_step,
                                        "per_launch": {"avg_launch_ms": round(avg_s * 1e3, 4), "launches": int(knn_n), "achieved": round(laneops_launch / avg_s / 1e12, 3),
                                                       "frac": round(laneops_launch / avg_s / 1e12 / VALU_PEAK_TLANEOPS, 4), "note": per_launch_note}}, **common)
            if prof_alone and prof_alone["knn"][1] > 0 and "roofline" in out:
                a_s = prof_alone["knn"][0] / prof_alone["knn"][1] * 1e-3
                unit_work = (2.0 * 256 if args.knn != "valu" else LANEOPS_PER_PAIR) * (pairs_alone / prof_alone["knn"][1]) / 1e12
                scale = M / max(Mk, 1)              # algorithmic (K x M) over executed (K x Mu) pairs; 1 for the VALU engine
                out["roofline"]["one_batch_in_flight"] = {
                    "avg_launch_ms": round(a_s * 1e3, 4), "achieved": round(unit_work / a_s, 2),
                    "frac": round(unit_work / a_s / out["roofline"]["peak"], 4),
                    "algorithmic_achieved": round(unit_work * scale / a_s, 2), "algorithmic_frac": round(unit_work * scale / a_s / out["roofline"]["peak"], 4),
                    "note": "same kernel and input, 3 launches after the timed region with nothing else on the GPU; "
                            "achieved / frac by the pairs evaluated as above, algorithmic_* by SURVEY 8(d)'s K x M pair count"}
        out["stage_ms_per_step"] = {k: round(ms / max(args.steps, 1), 3) for k, (ms, n) in prof.items()}
        if prof_alone:
            out["stage_ms_one_batch_in_flight"] = {k: round(ms / max(n, 1), 3) for k, (ms, n) in prof_alone.items()}
        # ORB stage: algorithmic bytes per frame = 3wh + 5*Pi + 3.6 kB * K
        ws = [fw]; hs = [fh]
        for l in range(1, cfg.nlevels):
            s = np.float32(np.float64(np.float32(cfg.scale_factor)) ** l)
            ws.append(int(np.rint(np.float32(fw) / s))); hs.append(int(np.rint(np.float32(fh) / s)))
        Pi = int(sum(a * b for a, b in zip(ws, hs)))
        orb_bytes = 3 * fw * fh + 5 * Pi + 3600 * float(v["n_keypoints"].mean())
        orb_ms = prof["orb"][0] / max(prof["orb"][1], 1)
        if orb_ms > 0:
            # the stage's interval inside the timed region is an occupancy figure too (it runs UNDER the other batches' search
            # kernels, one search block per CU, and lasts about a step): achieved / frac are the stage with the chip to itself
            # when that was measured, the timed region's interval is beside it
            rate = lambda ms: round(orb_bytes * U / (ms * 1e-3) / 1e9, 2)      # (a stage interval = one unit of U frames)
            alone_ms = prof_alone["orb"][0] / max(prof_alone["orb"][1], 1) if prof_alone and prof_alone["orb"][1] > 0 else 0.0
            ref_ms = alone_ms if alone_ms > 0 else orb_ms
            out["orb_stage"] = {"bound": "hbm", "algorithmic_bytes_per_frame": int(orb_bytes),
                                "achieved": rate(ref_ms), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(rate(ref_ms) / HBM_PEAK_GBS, 4),
                                "interval": "one batch in flight" if alone_ms > 0 else "timed region",
                                "in_timed_region": {"ms": round(orb_ms, 3), "achieved": rate(orb_ms), "frac": round(rate(orb_ms) / HBM_PEAK_GBS, 4)}}

    # ---- the drop-in path's rate: HOST frames in (what crates/matching-hip and every host mirror hand over), PCIe-inclusive —
    # never `value` (inputs are resident in HBM when the timed region starts); 1 warm-up + 3 calls on pinned memory, outside the
    # timed region (rank 0, N=1; --full)
    if args.full and rank == 0 and world == 1 and not args.no_host_frames:
        hf = torch.from_numpy(frames).pin_memory().numpy()
        hv = m.match_frames(hf)
        t0 = time.perf_counter()
        for _ in range(3):
            hv = m.match_frames(hf)
        dth = (time.perf_counter() - t0) / 3
        out["host_frames"] = {"value": round(len(hf) / dth, 1), "unit": "frames/s", "ms_per_call": round(dth * 1e3, 3), "frames_per_call": int(len(hf)),
                              "h2d_inclusive_GBps": round(hf.nbytes / dth / 1e9, 2), "memory": "pinned host memory",
                              "verdicts_equal_to_resident_run": bool(np.array_equal(hv["page_idx"][(np.arange(B) + g_last) % pool], v["page_idx"])) if B == pool == len(hf) else None,
                              "note": "slideo_match_frames_bgr8 on host frames: the H2D copy (one ordered copy stream, 32-frame units) is the bound; "
                                      "reported beside `value`, never as it"}
        del hf

    # ---- CPU baseline: the CPU restatement on the host cores, bounded sample (rank 0, N=1 only; --full)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import pyoracle
        ocfg = pyoracle.default_config(nfeatures=wl["nfeatures"], verify_model=verify_model, ocv_hdlt=args.hdlt, matcher=1 if args.matcher == "lsh" else 0,
                                       verdict_rule=args.verdict_rule)
        budget = host_cpu_budget()
        cores = max(1, min(ncpu, budget["usable"]))
        db = pyoracle.PageDB(ocfg)
        t0 = time.time()
        db.add_pages(pages, threads=cores)
        rc = db.finalize()
        t_cpu_db = time.time() - t0
        assert rc == 0 and db.descriptor_count == M, "CPU restatement and GPU page DB disagree"
        # one frame per thread (mirrors rayon's spawn_fifo, mo/lib.rs:213); the sample is the benchmark batch, repeated until the
        # leg has run for ~10 s so that start-up and the slowest thread do not dominate
        ns = min(args.cpu_sample or pool, pool)
        reps, t_cpu = 0, 0.0
        while t_cpu < 10.0 and reps < 20:
            t0 = time.time()
            cv = db.match_frames(frames[:ns], threads=min(cores, ns))
            t_cpu += time.time() - t0
            reps += 1
        # (resident frame j is the step's frame i with (g_last + i) mod pool == j)
        agree = float((cv["page_idx"] == v["page_idx"][(np.arange(ns) - g_last) % pool]).mean())
        n1 = 4
        t0 = time.time()
        db.match_frames(frames[:n1], threads=1)                      # also on one core
        t_cpu1 = time.time() - t0
        rate_n, rate_1, used = ns * reps / t_cpu, n1 / t_cpu1, int(min(cores, ns))
        simd = pyoracle.knn_hamming_blocked(np.zeros((1, 32), np.uint8), np.zeros((8, 32), np.uint8), 1)[2]
        out["cpu_baseline"] = {"value": round(rate_n, 3), "unit": "frames/s", "cores": used,
                               "kind": "port", "sample": "%d x the first %d benchmark frames, one frame per thread, page DB prebuilt (%.1f s on %d threads)" % (reps, ns, t_cpu_db, cores),
                               "seconds": round(t_cpu, 2), "verdict_agreement_with_gpu": agree,
                               "what": "exact brute-force restatement of the same path (oracle/: cache-blocked Hamming k-NN, %s); the reference's own CPU path searches a FLANN-LSH index instead (mo/flann.rs:16-21) and could not be built or timed here" % ("AVX-512 VPOPCNTDQ" if simd else "scalar popcnt"),
                               "single_thread": {"value": round(rate_1, 4), "unit": "frames/s", "cores": 1, "sample": "%d frames" % n1},
                               "thread_scaling": {"speedup": round(rate_n / rate_1, 1), "efficiency": round(rate_n / rate_1 / used, 3),
                                                  "host": budget,
                                                  "note": "%d threads; the host shows %d logical CPUs, the scheduler affinity %d, the cgroup quota %s "
                                                          "(SMT siblings share a core's vector units)" % (used, ncpu, budget["affinity"], budget["cgroup_quota_cpus"])}}
    if rank == 0:
        print(json.dumps(out), flush=True)
    m.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
