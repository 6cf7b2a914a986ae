#!/usr/bin/env python3
"""bench.py — registered images/sec (+ final Chamfer) of the image-sequence registration hot path.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One STEP = one pass of the hot path over this rank's batch of second-sequence images (BASELINE.json
configs[1]: 64 images of 640x480x64-D bf16 queries against 20 000 keys, per GPU):
  per image   getCors (K1) -> top-80 % filter -> correspondence assembly -> pnp(500, 2 px, P3P) (K2)
  per step    all-gather of the poses, the consecutive-pair Chamfer pick (K3) with one packed
              all-reduce(MIN), then on rank 0 the ICP refinement (K3/K4) and the final Chamfer
              against the CAD cloud for the picked image.
The rank's images sit in one (n, P, D) tensor; K1 is launched per --group images (they are
independent: grouping only lengthens the launch so its tail is ~2 % instead of ~20 %) on a stream of
its own, the per-image filter/RANSAC chains run on side streams beside the next K1 launch.
Inputs are synthetic (no BOP data or checkpoints exist offline), generated on the device before
the timed region; every timed byte is already resident in HBM.  Weak scaling: each rank owns
--images images, image i of the sequence lives on rank i // images.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps steps and prints the headline
(`value`, `ms_per_step`, the last step's final Chamfer); --dump-outputs DIR also writes what the last timed step
computed as DIR/<name>.npy (rank 0's view, float32 / float64).  Everything else is measured only with --full:
  roofline      K1 (the dominant kernel): algorithmic 2*P*N*D FLOP per launch / its average launch
                duration measured live with HIP events on the launch stream, against the dense
                bf16 MFMA peak; `traffic` from profiles/ (rocprofv3 --pmc) when committed.
  cpu_baseline  the CPU oracle (kind "port": the reference's own OpenCV/Open3D path cannot run
                here) timed on a bounded sample of the same workload on this box's host cores.
and, untimed, `parity_check` (the last step recomputed by the oracle) and `estimate_pose` (the reference's other per-image
path, poseEstSurf.estimate_pose, at its own size: ms per call of the matrix-free and of the materialised route) and
`reference_shape` (the reference's own 75 x 75 / 12-D / 80 000-key per-image loop through sequence.register_crops),
`acceptance`, `ransac_all_hypotheses`, `f32_step`, `screened_step`, `roofline_nn`, `roofline_ransac`, `nn_stage` and
`stage_ms_per_step`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

from imagesequenceregistrationfor6dposeestimationlabeling_amd import (  # noqa: E402
    ops, registration, sequence, shard, synth)

PEAK_BF16_MFMA = 2.5e15   # dense, MI355X_MICROARCH.md
PEAK_FP32_VALU = 157.3e12
PEAK_FP32_MFMA = 157.3e12  # dense f32 matrix peak, MI355X_MICROARCH.md


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--images", type=int, default=64, help="second-sequence images per GPU")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--keys", type=int, default=20000)
    ap.add_argument("--itr", type=int, default=500)
    ap.add_argument("--cad", type=int, default=5000)
    ap.add_argument("--streams", type=int, default=3, help="HIP streams the images are pipelined over")
    ap.add_argument("--group", type=int, default=32, help="images per K1 launch (1 = one launch per image)")
    ap.add_argument("--refine-iters", type=int, default=6, help="Gauss-Newton refit iterations after RANSAC")
    ap.add_argument("--k1", choices=("log2", "natural", "screened"), default="log2",
                    help="log2: descriptors multiplied by log2(e) before their one rounding to bf16 "
                         "(ISR_DTYPE_BF16_LOG2, the direct-sum kernel); natural: plain bf16 (ISR_DTYPE_BF16); screened: the log2 "
                         "rows behind the FP6 screen (ISR_DTYPE_BF16_LOG2_SCREENED, round 5) — pays only where the softmax is "
                         "peaked beyond f32 resolution (--tau >= 7); at the bench's tau = 5 every term of the sums counts, the "
                         "screen can skip nothing and the call costs 1.4 x the unscreened one (profiles/r05_k1_screen.txt)")
    ap.add_argument("--tau", type=float, default=5.0, help="descriptor norm |k| (softmax sharpness), see make_model")
    ap.add_argument("--depth", type=int, default=1,
                    help="how many batches the registration may run ahead of the verification (step overlap)")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="finish a step's ICP + final Chamfer before the next step's registration starts")
    ap.add_argument("--epilogue-digits", action="store_true",
                    help="A/B: K1 forms the cut's first histogram in its epilogue (isr_corr_argmax_digits + "
                         "isr_select_top_batch_digits, SURVEY 8(f)-2) instead of the plain isr_corr_argmax + ten-launch "
                         "isr_select_top_batch pair; same results, 5 %% slower (profiles/r05_epilogue_histogram_ab.txt)")
    ap.add_argument("--k1-one-call", action="store_true",
                    help="A/B: one isr_corr_argmax call per group on the K1 stream (sequence.K1_SPLIT_CLOSE = False) instead of the "
                         "call's closing kernels on the group's side stream (isr_corr_argmax_phase)")
    ap.add_argument("--host-gc", action="store_true", help="leave Python's cyclic garbage collector enabled during the timed steps")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--confidence", type=float, default=0.99,
                    help="RANSAC confidence (cv2.solvePnPRansac's parameter; its default 0.99 is what the reference's "
                         "call uses); 1 scores every hypothesis")
    ap.add_argument("--icp-iters", type=int, default=30, help="debug only (not a valid bench line): the ICP's iteration cap (Open3D's default 30)")
    ap.add_argument("--ablate", default="", help="debug only (not a valid bench line): 'noverify' skips a13-a15")
    ap.add_argument("--tune", default="", help="debug only (not a valid bench line): library knobs, e.g. 'nn_plan_rq=1,icp_warm=0' (ops.set_tuning)")
    ap.add_argument("--cpu-threads", type=int, default=16, help="host threads for the cpu_baseline leg")
    ap.add_argument("--verify", choices=("pick", "vote"), default="pick",
                    help="verification stage: 'pick' = consecutive-pair Chamfer pick (verfication.py:61-108, the headline); "
                         "'vote' = the n x n ADD-S vote whose top choice icp.py:37-39 reads (choosePose.py:121-151)")
    ap.add_argument("--object", choices=("tless", "revolution"), default="tless",
                    help="tless: the discrete-symmetric box with a boss (configs[1]/[2]); revolution: the continuous-symmetry "
                         "surface of revolution of BASELINE configs[3], descriptors constant along the azimuth up to a weak term")
    ap.add_argument("--no-estimate-pose", action="store_true", help="skip the untimed estimate_pose / reference-shape timings")
    ap.add_argument("--no-parity-check", action="store_true", help="skip the untimed oracle re-computation of the last step")
    ap.add_argument("--no-f32-step", action="store_true", help="skip the untimed step on f32 descriptors (the reference's precision)")
    ap.add_argument("--no-screened-step", action="store_true", help="skip the untimed |k| = 8 step pair (K1 unscreened / behind the FP6 screen)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: per-kernel timing inside the timed steps, rooflines, the untimed extra steps "
                         "(all hypotheses, f32, |k| = 8), acceptance, parity check, estimate_pose / reference shape, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


# K1's per-query outputs of one image are dumped whole up to this many rows, beyond it as a fixed sorted sample
DUMP_K1_ROWS = 1 << 20


def dump_outputs(out_dir: str, last: dict) -> None:
    """What the last timed step handed back on rank 0, one .npy per array: every image's pose (all-gathered), this rank's
    RANSAC status, K1's arg-max / log-probability for this rank's first image, the verification's result and the ICP +
    final Chamfer of the picked image.  float64 throughout, except K1's f32 log-probabilities."""
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    arrs = {"poses": np.asarray(last["poses_all"], np.float64).reshape(-1, 3, 4)} if "poses_all" in last else {}
    if "_status_local" in last:
        arrs["status"] = last["_status_local"].cpu().numpy().astype(np.float64)
    if last.get("_k1_first") is not None:
        idx, logp = (t.cpu().numpy() for t in last["_k1_first"])
        rows = np.arange(idx.shape[0])
        if rows.size > DUMP_K1_ROWS:
            rows = np.sort(np.random.default_rng(0).choice(rows.size, DUMP_K1_ROWS, replace=False))
            arrs["k1_rows"] = rows.astype(np.float64)
        arrs["k1_idx"] = idx[rows].astype(np.float64)
        arrs["k1_logp"] = logp[rows].astype(np.float32)
    if last.get("chamfer_table") is not None:
        arrs["chamfer_table"] = np.asarray(last["chamfer_table"], np.float64)
    for k in ("picked_image", "final_chamfer", "icp_fitness", "icp_rmse"):
        if last.get(k) is not None:
            arrs[k] = np.array([last[k]], np.float64)
    if last.get("_icp_T") is not None:
        arrs["icp_T"] = np.asarray(last["_icp_T"], np.float64).reshape(4, 4)
    for name, a in arrs.items():
        np.save(d / f"{name}.npy", a)


def make_model(dev, N, D, tau=5.0, obj="tless"):
    """Keys with |k| = tau.  tau sets how peaked the softmax is: at tau = 8 (SURVEY's first suggestion) a
    planted query beats the log-sum of the other 20 000 keys by > 30 nats, EVERY log-probability is 0
    to f32 rounding, and the top-80 % cut (strict `>` on exact ties, inference.py:282-290) keeps
    nothing — in the reference's own torch f32 log_softmax as much as here.  tau = 5 leaves a 10-nat
    margin: log-probabilities spread over 1e-6 .. 1e-2 and the cut does real work."""
    rng = np.random.default_rng(20240)
    solid = synth.revolution if obj == "revolution" else synth.tless_like
    pts = solid(rng, N)
    if obj == "revolution":
        # configs[3]: keys of points on one parallel are nearly identical (synth.revolution_keys) — correspondences are
        # ambiguous about the azimuth by construction, RANSAC sees a low inlier ratio
        keys_f32 = torch.from_numpy(synth.revolution_keys(rng, pts, D, tau=tau)).to(dev)
    else:
        g = torch.Generator(device=dev).manual_seed(777)
        k = torch.randn(N, D, device=dev, generator=g)
        keys_f32 = tau * k / k.norm(dim=1, keepdim=True)
    cloud = solid(rng, 4 * N)
    upper, lower = synth.split_halves(rng, cloud, N)
    # the two halves are kept in Morton order (rows that are neighbours in space): a rigid motion keeps that locality, so the
    # ICP's per-wave tile cull works on them as stored and the calls below pass spatial_order=False (no sort per step)
    upper = upper[registration.morton_order(torch.from_numpy(upper)).numpy()]
    lower = lower[registration.morton_order(torch.from_numpy(lower)).numpy()]
    cad = solid(rng, 5000)
    return keys_f32, torch.from_numpy(pts).to(dev), upper, lower, cad


def make_image(dev, keys_f32, pts, Kcam, R, t, P, seed, log2_domain=True):
    """Device-side twin of synth.image_case (same recipe, torch RNG): planted descriptors with
    30 % wrong matches, pixel = projection of the true point + 0.5 px noise.  log2_domain: the f32
    descriptors are multiplied by log2(e) BEFORE the one rounding to bf16 (ISR_DTYPE_BF16_LOG2)."""
    N = keys_f32.shape[0]
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    gt_geo = torch.randint(N, (P,), device=dev, generator=g)
    out = torch.rand(P, device=dev, generator=g) < 0.3
    gt_match = torch.where(out, torch.randint(N, (P,), device=dev, generator=g), gt_geo)
    Q = keys_f32[gt_match] + 0.35 * torch.randn(P, keys_f32.shape[1], device=dev, generator=g)
    Q = ops.prescale_queries_log2(Q) if log2_domain else Q.bfloat16()
    Rt = torch.from_numpy(np.concatenate([R, t[:, None]], 1)).to(dev)
    Xc = pts[gt_geo].double() @ Rt[:, :3].T + Rt[:, 3]
    p = Xc @ torch.from_numpy(Kcam).to(dev).T
    pix = (p[:, :2] / p[:, 2:3] + 0.5 * torch.randn(P, 2, device=dev, generator=g, dtype=torch.float64)).float()
    return Q.contiguous(), pix.contiguous()


def _median_time(fn, reps=5):
    """One warm-up call, then the median of `reps` timed calls."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def cpu_baseline(args, keys_bf16, pts, Q0, pix0, Kcam, upper, lower, cad, R_gt, t_gt):
    """The CPU oracle ("port": the reference's own OpenCV / Open3D calls cannot run here) on ONE image's share of the step,
    scaled to images/s.  Round 4: every leg runs at the image's FULL size — getCors over all P rows (one repetition on all
    cores, ~10 s; the one-core figure extrapolates a 4 096-row sample), the filter, the n_eval P3P hypotheses the staged loop
    scores at the bench's confidence, their scoring against all 0.8 P correspondences, the refit over the inliers, one
    Chamfer pair, ICP + final Chamfer / images.  Per leg: one warm-up + median of 5 (getCors full: 1; ICP: 3)."""
    from oracle import cbind, pnp_oracle, registration_oracle as ro
    try:
        from threadpoolctl import threadpool_limits
    except Exception:                      # pragma: no cover
        threadpool_limits = None
    # the box exposes every host core but a 1-GPU job's share is 16 (see the task's Environment notes)
    cores = min(len(os.sched_getaffinity(0)), args.cpu_threads)
    P, N = Q0.shape[0], keys_bf16.shape[0]
    Ps = min(P, 4096)
    scale = ops.LOG2E if args.k1 != "natural" else 1.0
    q_full = Q0.float().cpu() / scale
    q = q_full[:Ps]
    k = keys_bf16.float().cpu()
    idx, vals = ro.getCors_chunked(q, k, chunk=4096)
    full_vals = vals.repeat((P + Ps - 1) // Ps, 1)[:P]
    M = int(0.8 * P)                                     # what the top-80 % cut hands to pnp
    rep = (M + Ps - 1) // Ps
    p3d = pts.cpu().numpy()[np.tile(idx.numpy(), rep)[:M] % N]        # the sample's matches, tiled: the legs' cost does not depend on the values
    p2d = np.tile(pix0[:Ps].cpu().numpy(), (rep, 1))[:M]
    # how many hypotheses the staged RANSAC loop scores on this data: the oracle with the bench's confidence
    o = pnp_oracle.pnp_ransac(p3d[:20000], p2d[:20000], Kcam, H=args.itr, reperr=2.0, seed=1, refine_iters=0, confidence=args.confidence)
    n_eval = int(o["n_eval"])
    Rt, ok, _ = pnp_oracle.hypotheses(p3d, p2d, Kcam, n_eval, 1)
    inl = np.zeros(M, bool)
    inl[: int(0.7 * M)] = True                           # 30 % wrong matches in the data
    pc = pts.cpu().numpy().astype(np.float64)
    src = (upper.astype(np.float64) @ R_gt[0].T + t_gt[0]).astype(np.float32)
    init = np.linalg.inv(np.vstack([np.hstack([R_gt[0], t_gt[0][:, None]]), [0, 0, 0, 1]]))

    def icp_and_final():
        T, _, _, _ = ro.icp_point_to_point(src, lower, 20, init)
        ro.final_chamfer(src, lower, T, cad)

    def legs(full_getcors):
        t = {}
        if full_getcors:
            t0 = time.perf_counter()
            ro.getCors_chunked(q_full, k, chunk=4096)
            t["getCors"] = time.perf_counter() - t0
        else:
            t["getCors"] = _median_time(lambda: ro.getCors_chunked(q, k, chunk=4096)) * (P / Ps)
        t["filter"] = _median_time(lambda: ro.filter_top(full_vals))
        t["p3p"] = _median_time(lambda: pnp_oracle.hypotheses(p3d, p2d, Kcam, n_eval, 1))
        t["score"] = _median_time(lambda: cbind.ransac_score(p3d, p2d, Kcam, Rt, ok, 2.0))
        t["refit"] = _median_time(lambda: pnp_oracle.refine(p3d, p2d, Kcam, Rt[0], inl, iters=args.refine_iters), reps=3)
        t["chamfer_pair"] = _median_time(lambda: ro.chamfer(pc @ R_gt[0].T, pc @ R_gt[1].T))
        t["icp_share"] = _median_time(icp_and_final, reps=3) / args.images
        return t

    out = {}
    for label, n in (("all_cores", cores), ("one_core", 1)):
        torch.set_num_threads(n)
        os.environ["OMP_NUM_THREADS"] = str(n)
        if threadpool_limits is not None:
            with threadpool_limits(limits=n):
                t = legs(n > 1)
        else:
            t = legs(n > 1)
        out[label] = {"images_per_s": 1.0 / sum(t.values()), "cores": n, "seconds_per_image": t}
    torch.set_num_threads(cores)
    return {
        "value": out["all_cores"]["images_per_s"], "unit": "images/s", "cores": cores, "kind": "port",
        "one_core_value": out["one_core"]["images_per_s"],
        "protocol": "per leg: 1 warm-up + median of 5 (refit, ICP: 3; the full-size getCors: 1 repetition)",
        "sample": (f"1 image at full size: getCors on all {P} query rows (torch-CPU f32, {cores} threads, measured; the one-core "
                   f"figure extrapolates {Ps} rows x{P / Ps:.0f}); filter on all {P} values; the {n_eval} of {args.itr} NumPy P3P "
                   f"hypotheses the staged loop scores at confidence {args.confidence} + C scoring of them against all {M} "
                   f"correspondences; GN refit ({args.refine_iters} its) over {int(0.7 * M)} inliers; 1 cKDTree Chamfer pair of "
                   f"{N} points; ICP + final Chamfer / {args.images} images"),
        "legs": out,
    }


def measure_nn(pts, dev, pairs=32):
    """K3 brute force (nn_search_kernel, ISR_TUNE_NN_PATH = 0) on `pairs` Chamfer-pair items of N x N points with
    unrelated orientations, timed with HIP events on the launch stream.  Three figures:
    the VALU fraction under the 8-FLOP/pair convention, the algorithmic bytes against HBM, and — from
    the committed PMC run, when there is one for this shape — the counter HBM bytes."""
    N = pts.shape[0]
    rng = np.random.default_rng(5)
    Ra, ta = synth.random_poses(rng, pairs)
    Rb, tb = synth.random_poses(rng, pairs)
    Tq = torch.from_numpy(np.concatenate([Ra, np.zeros((pairs, 3, 1))], 2)).to(dev)
    Tt = torch.from_numpy(np.concatenate([Rb, np.zeros((pairs, 3, 1))], 2)).to(dev)
    with ops.tuning(nn_path=0):          # explicit knob, no environment access (no other thread is running here)
        ops.nn_batched(pts, pts, Tq, Tt)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(3):
            ops.nn_batched(pts, pts, Tq, Tt)
        e1.record()
        torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) * 1e-3 / 3
    n_pairs = float(pairs) * N * N
    alg_bytes = 12.0 * N + 12.0 * N + 96.0 * pairs + 8.0 * N * pairs
    pmc = ROOT / "profiles" / "nn_hbm_traffic.json"
    counter = None
    if pmc.exists():
        rec = json.loads(pmc.read_text()).get(f"{N}x{N}x{pairs}")
        counter = rec["hbm_bytes"] if rec else None
    return {"kernel": "nn_search_kernel<4> + nn_finalize_kernel (brute force)", "shape": f"{pairs} items of {N} x {N}",
            "ms": sec * 1e3, "pairs_per_s": n_pairs / sec, "bound": "f32 VALU (8 FLOP/pair convention)",
            "valu_frac": 8.0 * n_pairs / sec / PEAK_FP32_VALU, "algorithmic_bytes": alg_bytes,
            "algorithmic_hbm_frac": alg_bytes / sec / 8.0e12,
            "counter_hbm_bytes": counter, "counter_hbm_frac": (counter / sec / 8.0e12) if counter else None,
            "counter_source": "profiles/nn_hbm_traffic.json (rocprofv3 --pmc, separate run)" if counter else None}


def measure_ransac(dev, pts, Kcam, M=245760, H=4096, reps=5):
    """K2 alone (BASELINE configs[3]'s hypothesis count): isr_ransac_score — every one of H P3P
    hypotheses scored against M correspondences (0.8 x 640 x 480), HIP events on the launch stream.  The entry is
    proj_matrix_kernel + ONE score_kernel launch + best_kernel + best_mask_kernel; score_kernel is > 95 % of it
    (profiles/r04_k2_*).  FLOPs by the survey's convention: 30 per (hypothesis, correspondence); algorithmic bytes
    20 M + 48 H + 4 H + M / 8."""
    rng = np.random.default_rng(4)
    R, t = synth.random_poses(rng, 1)
    p3d, p2d, _ = synth.pnp_case(rng, pts.cpu().numpy(), Kcam, R[0], t[0], M)
    p3, p2 = torch.from_numpy(p3d).to(dev), torch.from_numpy(p2d).to(dev)
    Rt, ok = ops.p3p_hypotheses(p3, p2, Kcam, H, seed=11)[:2]
    n_inl, best, _ = ops.ransac_score(p3, p2, Kcam, Rt, ok, 2.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        n_inl, best, _ = ops.ransac_score(p3, p2, Kcam, Rt, ok, 2.0)
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) * 1e-3 / reps
    n_ok = int(ok.sum().item())
    pairs = float(n_ok) * M                      # hypotheses whose P3P failed are skipped by the kernel: not counted
    alg_bytes = 20.0 * M + 52.0 * H + M / 8.0
    return {"kernel": "isr_ransac_score: proj_matrix_kernel + score_kernel (one launch, every hypothesis) + best_kernel + "
                      "best_mask_kernel", "shape": f"H = {H} hypotheses ({n_ok} with a P3P solution) x M = {M} correspondences",
            "ms": sec * 1e3, "hyp_corr_per_s": pairs / sec, "bound": "f32 VALU (30 FLOP per hypothesis-correspondence pair, "
            "SURVEY 8(d))", "achieved": 30.0 * pairs / sec * 1e-12, "peak": PEAK_FP32_VALU * 1e-12, "unit": "TFLOP/s",
            "frac": 30.0 * pairs / sec / PEAK_FP32_VALU, "algorithmic_bytes": alg_bytes,
            "algorithmic_hbm_frac": alg_bytes / sec / 8.0e12, "best_hypothesis": int(best.item()),
            "best_inliers": int(n_inl[int(best.item())].item())}


def measure_k1_f32(Q_img, keys_f32, dev, log2_domain):
    """K1 at the reference's own precision (f32 descriptors, the reference's f32 matmul, inference.py:142-149) on ONE image
    of the workload.  Default route at D <= 64 since round 4: every f32 number as f16 planes x1 | x2s | x1s, three plane
    pairs per 16-wide block on the f16 matrix cores, margin test + recheck by the f32 fmaf chain — the indices of the chain
    kernel bit for bit, log-probabilities to f32 accuracy — priced against the f32 matrix peak (what a plain f32 GEMM could
    reach) and, as matrix instructions actually issued, against the 16-bit peak.  Beside it the bf16-plane form (six plane
    pairs, ISR_TUNE_K1_F32_CHAIN = 2) and the f32-MFMA chain kernel (= 1), round 3's only route for D > 16."""
    q = Q_img.float() / (ops.LOG2E if log2_domain else 1.0)
    D = q.shape[1]
    flop = 2.0 * q.shape[0] * keys_f32.shape[0] * D

    def timed(chain, reps=3):
        with ops.tuning(k1_f32_chain=chain):
            ops.corr_argmax(q, keys_f32)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                out = ops.corr_argmax(q, keys_f32)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps, out, ops.corr_recheck_count_f32(D)

    ms, out, rechecked = timed(0)
    ms_bf, out_bf, _ = timed(2)
    ms_chain, out_chain, _ = timed(1)
    planes = rechecked >= 0
    Dp = 16 if D <= 16 else 32 if D <= 32 else 64
    issued = 3.0 * flop * Dp / D                      # f16 planes: three plane pairs per 16-wide block, padded width Dp
    return {"kernel": ("corr_bf16_direct_kernel<.., SP, F16> (f16 planes of the f32 rows, 3 plane pairs per block, exact f32-chain "
                       "recheck)" if planes else "corr_f32_kernel (exact f32 MFMA path)"),
            "ms_per_image": ms,
            # a roofline fraction is ISSUED work over the peak of the pipe it is issued on (round 4 divided the useful f32 FLOPs by
            # the f32 matrix peak for a kernel that runs on the 16-bit pipe: 2.03, not a fraction)
            "bound": "mfma (16-bit pipe)" if planes else "mfma (f32 pipe)",
            "achieved": (issued if planes else flop) / (ms * 1e-3) * 1e-12, "peak": (PEAK_BF16_MFMA if planes else PEAK_FP32_MFMA) * 1e-12,
            "unit": "TFLOP/s", "frac": (issued / PEAK_BF16_MFMA if planes else flop / PEAK_FP32_MFMA) / (ms * 1e-3),
            "useful_f32_tflops": flop / (ms * 1e-3) * 1e-12,
            "useful_f32_flops_over_f32_matrix_peak": flop / (ms * 1e-3) / PEAK_FP32_MFMA,
            "queries_decided_by_f32_chain_recheck": rechecked,
            "bf16_planes": {"ms_per_image": ms_bf, "frac": 6.0 * flop * Dp / D / (ms_bf * 1e-3) / PEAK_BF16_MFMA,
                            "useful_f32_flops_over_f32_matrix_peak": flop / (ms_bf * 1e-3) / PEAK_FP32_MFMA,
                            "idx_equal": bool(torch.equal(out[0], out_bf[0]))},
            "f32_mfma_chain_kernel": {"ms_per_image": ms_chain, "achieved": flop / (ms_chain * 1e-3) * 1e-12,
                                      "frac": flop / (ms_chain * 1e-3) / PEAK_FP32_MFMA},
            "idx_equal_chain_kernel": bool(torch.equal(out[0], out_chain[0])),
            "logp_max_abs_diff_vs_chain": float((out[1] - out_chain[1]).abs().max())}


def rank_command(n: int, port: int, argv: list) -> list:
    """The child command of a plain `python bench.py --gpus N`: the driver's own launch line (one rank per GPU of one node)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve()), *argv]


def spawn_ranks(n: int) -> int:
    """`python bench.py --gpus N` started plainly: run the N ranks as CHILD processes under
    torch.distributed.run (one per GPU) and relay their output.  Nothing in this process has touched the
    GPU yet, and it never replaces itself (no exec): it waits for the children and returns their code."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = rank_command(n, port, sys.argv[1:])
    print("bench.py: launching " + " ".join(cmd), file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")).returncode


def measure_nn_vote(cad_d, pts, dev, items=4096):
    """K3 at the vote's shape (choosePose.py:121-138): `items` ADD-S items of V CAD vertices against N surface points,
    brute force (the vote's items take nn_search_kernel: queries sit far from their targets), HIP events."""
    V, N = cad_d.shape[0], pts.shape[0]
    rng = np.random.default_rng(6)
    Ra, ta = synth.random_poses(rng, items, tz=0.0, t_sigma=2.0)
    Rb, tb = synth.random_poses(rng, items, tz=0.0, t_sigma=2.0)
    Tq = torch.from_numpy(np.concatenate([Ra, ta[:, :, None]], 2)).to(dev)
    Tt = torch.from_numpy(np.concatenate([Rb, tb[:, :, None]], 2)).to(dev)
    ops.nn_batched(cad_d, pts, Tq, Tt)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(2):
        ops.nn_batched(cad_d, pts, Tq, Tt)
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) * 1e-3 / 2
    n_pairs = float(items) * V * N
    alg_bytes = 12.0 * V + 12.0 * N + 192.0 * items
    return {"kernel": "isr_nn_batched on the vote's items (default plan)", "shape": f"{items} items of {V} x {N}",
            "ms": sec * 1e3, "pairs_per_s": n_pairs / sec, "bound": "f32 VALU (8 FLOP/pair convention)",
            "valu_frac": 8.0 * n_pairs / sec / PEAK_FP32_VALU, "algorithmic_bytes": alg_bytes,
            "algorithmic_hbm_frac": alg_bytes / sec / 8.0e12}


def parity_check(args, model, Q_rows, keys, pts, last, R_gt, t_gt, upper, lower, cad, max_pairs=1023):
    """UNTIMED tail, rank 0: what the last timed step produced, recomputed by the CPU oracle (round-2 verdict:
    the bench's own pick / ICP / final Chamfer had never been compared with anything).
      * K1: the arg-max of 1 024 query rows of the first image against oracle/isr_oracle.c (exact bf16 products);
      * pick: EVERY consecutive-pair Chamfer value of the last step (all n - 1 pairs up to `max_pairs` = 1 023, i.e. all
        511 of configs[2]; beyond that a sample with the picked pair in it, and then `pick_idx_equal` is not reported —
        only `pick_is_min_of_sampled`) against the f64 cKDTree oracle, and the same first minimum (verfication.py:61-108);
      * ICP + final Chamfer for the picked image (icp.py:83-117) against the oracle loop with exact f64 neighbours
        (cKDTree; the device flags near ties of its f32 search and decides them in f64: DESIGN.md K3/K4)."""
    from oracle import cbind, registration_oracle as ro
    out = {}
    rows = min(1024, Q_rows.shape[0])
    step = max(1, Q_rows.shape[0] // rows)
    q = Q_rows[::step][:rows].contiguous()
    idx_dev, _ = ops.corr_argmax(q, keys, log2_prescaled=model.log2_queries, screened=model.screened)
    bits = lambda x: x.cpu().view(torch.int16).numpy().view(np.uint16)
    o = cbind.corr_argmax_bf16(bits(q), bits(keys), logit_scale=float(np.log(2.0)) if model.log2_queries else 1.0)
    out["k1_rows_checked"] = int(rows)
    out["k1_idx_equal_rows"] = int((idx_dev.cpu().numpy() == o["idx"]).sum())
    if last.get("_k1_first") is not None:
        # what the LAST TIMED STEP's K1 launch (32 images per launch, beside the chains and the verification) left for this
        # rank's first image, against the same rows through a launch of their own with the GPU idle: a result is a function
        # of (query, keys) only, so both must be the same bits
        idx_step, logp_step = last["_k1_first"]
        idx_alone, logp_alone = ops.corr_argmax(Q_rows, keys, log2_prescaled=model.log2_queries, screened=model.screened)
        out["k1_in_step_equals_alone"] = bool(torch.equal(idx_step, idx_alone) and torch.equal(logp_step, logp_alone))
    poses = np.asarray(last["poses_all"], np.float64).reshape(-1, 3, 4)
    n = poses.shape[0]
    pc = pts.cpu().numpy().astype(np.float64)
    if last.get("chamfer_table") is not None:
        table = np.asarray(last["chamfer_table"], np.float64)
        picked = int(last["picked_pair"])
        sel = np.arange(n - 1) if n - 1 <= max_pairs else np.unique(np.concatenate(
            [np.linspace(0, n - 2, max_pairs - 1).astype(int), [picked]]))
        ref = np.array([ro.chamfer(pc.dot(poses[i + 1, :, :3]),
                                   pc.dot(poses[i, :, :3].T).dot(ro.calculate_relative_pose(R_gt[i], t_gt[i], R_gt[i + 1], t_gt[i + 1])[0]))
                        for i in sel])
        out["pairs_checked"] = int(len(sel))
        out["pairs_total"] = int(n - 1)
        out["chamfer_max_abs"] = float(np.max(np.abs(table[sel] - ref)))
        out["table_argmin_equals_pick"] = bool(int(np.argmin(table)) == picked)
        if len(sel) == n - 1:
            out["pick_idx_equal"] = bool(int(np.argmin(ref)) == picked)
        else:
            out["pick_is_min_of_sampled"] = bool(ref[list(sel).index(picked)] == ref.min())
    best = int(last["picked_image"])
    pose = poses[best]
    src = (upper.astype(np.float64) @ R_gt[best].T + t_gt[best]).astype(np.float32)
    init = np.linalg.inv(np.vstack([pose, [0, 0, 0, 1]]))
    T, fit, rmse = registration.icp_point_to_point(src, lower, 20, init, spatial_order=False)
    fc = registration.final_chamfer(src, lower, T, cad)
    Tr, rfit, rrmse, traj = ro.icp_point_to_point(src, lower, 20, init, search="f64")
    out["icp_rot_rad"] = synth.rot_angle(T[:3, :3], Tr[:3, :3])
    out["icp_trans_mm"] = float(np.linalg.norm(T[:3, 3] - Tr[:3, 3]))
    out["icp_iterations"] = int(len(traj) - 1)
    out["final_chamfer_abs"] = float(abs(fc - ro.final_chamfer(src, lower, Tr, cad)))
    out["icp_fitness_abs"] = float(abs(fit - rfit))
    out["icp_rmse_abs"] = float(abs(rmse - rrmse))
    out["final_chamfer_device"] = fc
    out["note"] = ("oracle = oracle/ (C restatement of getCors; cKDTree exact f64 neighbours + Kabsch/SVD for the Chamfer values "
                   "and the ICP loop — Open3D's documented behaviour restated, unpinned: Open3D absent)")
    return out


def measure_reference_shape(dev, n=128, group=128, reps=4):
    """The reference's OWN per-image loop shape (inference.py:163, 248-293; genFeat.py:201): 224 x 224 crops -> 75 x 75
    lattice of ~2 200 masked pixels, 12-D f32 descriptors, 80 000 keys, 500 P3P hypotheses, through
    sequence.register_crops (one K1 launch + one filter / RANSAC chain per group of crops).  Untimed region; not `value`."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import sequence, synth
    cb = synth.crop_batch(dev, n)
    cams = np.broadcast_to(cb["Kc"], (n, 3, 3))
    out = {"shape": {"crop": 224, "lattice": cb["S1"], "masked_pixels_mean": float(np.mean(cb["counts"])), "D": cb["D"],
                     "N": int(cb["keys"].shape[0]), "itr": 500, "crops_per_group": group}, "unit": "images/s"}
    for label, model in (("f32_exact", sequence.SequenceModel(keys=cb["keys"], pts=cb["pts"])),
                         ("bf16", sequence.SequenceModel(keys=cb["keys"].bfloat16(), pts=cb["pts"], log2_queries=True))):
        kw = dict(n_feat=cb["D"], down_sample=cb["ds"], itr=500, seeds=list(range(n)), refine_iters=6, group=group)
        res, _ = sequence.register_crops(model, cb["feats"], cb["masks"], cams, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            res, _ = sequence.register_crops(model, cb["feats"], cb["masks"], cams, **kw)
        torch.cuda.synchronize()
        out[label] = reps * n / (time.perf_counter() - t0)
        errs = [synth.rot_angle(res[i].pose.cpu().numpy()[:, :3], cb["R"][i]) for i in range(n) if int(res[i].status.item())]
        out[label + "_registered"] = len(errs)
        out[label + "_median_rot_err_rad"] = float(np.median(errs)) if errs else None
    return out


def measure_estimate_pose(dev, reps=5):
    """The other per-image path (poseEstSurf.py:11-261) at the reference's own size — a 224 x 224
    crop, 12-D descriptors, 80 000 surface points, 10 000 samples, <= 1 000 scored poses: wall time per call of the
    matrix-free route (the default) and of the route through the materialised (n, m) matrices, which return the same bits.
    Untimed region of the bench; not part of `value`."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import pose_est_surf as pes, synth
    s = synth.crop_scene()
    a = [torch.from_numpy(s["mask_lgts"]).to(dev), torch.from_numpy(s["query"]).to(dev), torch.from_numpy(s["pts"]).to(dev),
         torch.from_numpy(s["normals"]).to(dev), torch.from_numpy(s["keys"]).to(dev), s["diameter"], s["K"]]
    out = {"shape": {"r": 224, "e": 12, "m": 80000, "max_poses": 10000, "max_pose_evaluations": 1000, "down_sample_scale": 3},
           "unit": "ms per call (wall, inputs resident)"}
    ref = {}
    for avg in (True, False):
        for mat in (False, True):
            kw = dict(max_poses=10000, max_pose_evaluations=1000, avg_queries=avg, seed=3, materialize=mat)
            res = pes.estimate_pose(*a, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                res = pes.estimate_pose(*a, **kw)
            torch.cuda.synchronize()
            key = f"avg_queries_{str(avg).lower()}" + ("_materialized" if mat else "")
            out[key] = (time.perf_counter() - t0) / reps * 1e3
            if not mat:
                ref[avg] = res
                out[f"poses_scored_avg_queries_{str(avg).lower()}"] = int(res[0].shape[0])
            else:
                out[f"routes_bit_identical_avg_queries_{str(avg).lower()}"] = bool(
                    all(torch.equal(x, y) if torch.is_tensor(x) else np.array_equal(x, y) for x, y in zip(ref[avg], res)))
    B = 32                              # a block of crops (the reference's loop over frames): estimate_poses
    ml, q = a[0][None].expand(B, -1, -1).contiguous(), a[1][None].expand(B, -1, -1, -1).contiguous()
    for avg in (True, False):
        kw = dict(max_poses=10000, max_pose_evaluations=1000, avg_queries=avg)
        pes.estimate_poses(ml, q, a[2], a[3], a[4], a[5], a[6], n_streams=2, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            pes.estimate_poses(ml, q, a[2], a[3], a[4], a[5], a[6], n_streams=2, **kw)
        torch.cuda.synchronize()
        out[f"block_of_{B}_ms_per_image_avg_queries_{str(avg).lower()}"] = (time.perf_counter() - t0) / (2 * B) * 1e3
    return out


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))
    rank, world, local = shard.init_from_env()
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        raise SystemExit(f"bench.py (rank {rank}): needs a HIP device — there is no CPU fallback for the hot path")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    P, N, D = args.width * args.height, args.keys, args.dim
    n_local, n_total = args.images, args.images * world
    if args.epilogue_digits:
        sequence.EPILOGUE_DIGITS = True
    if args.k1_one_call:
        sequence.K1_SPLIT_CLOSE = False
    if args.tune:
        ops.set_tuning(**{k: int(v) for k, v in (kv.split("=") for kv in args.tune.split(","))})
    Kcam = synth.camera(args.width, args.height)
    keys_f32, pts, upper, lower, cad = make_model(dev, N, D, args.tau, args.object)
    keys = keys_f32.bfloat16().contiguous()
    model = sequence.SequenceModel(keys=keys, pts=pts, log2_queries=args.k1 != "natural", screened=args.k1 == "screened")
    cad_d = torch.from_numpy(cad).to(dev)
    diameter = synth.diameter(pts.cpu().numpy())
    rng = np.random.default_rng(99)
    R_gt, t_gt = synth.random_poses(rng, n_total)          # every rank knows every GT pose (scene_gt.json)
    lo, hi = shard.block_range(n_total, rank, world)
    # the rank's block of images lives in ONE tensor (n, P, D) / (n, P, 2): K1 is launched per group
    Q_all = torch.empty((n_local, P, D), dtype=torch.bfloat16, device=dev)
    pix_all = torch.empty((n_local, P, 2), dtype=torch.float32, device=dev)
    for j, i in enumerate(range(lo, hi)):
        Q_all[j], pix_all[j] = make_image(dev, keys_f32, pts, Kcam, R_gt[i], t_gt[i], P, i, args.k1 != "natural")
    images = [(Q_all[j], pix_all[j]) for j in range(n_local)]
    torch.cuda.synchronize()

    def register(s: int, confidence: float):
        """Every rank: its block of images through a1-a5.  Enqueue only — returns the device tensors and
        an event that fires when the poses are complete.  Consecutive steps alternate between two
        issuing streams: the driver makes its issuing stream wait for every chain of the step, and
        the next step's first K1 launch must not inherit that wait."""
        with torch.cuda.stream(reg_streams[s & 1]):
            if args.group > 1:
                res = sequence.register_block(cur["model"], cur["Q"], pix_all, Kcam, itr=args.itr, reperr=2.0,
                                              seed0=(s << 20) + lo, refine_iters=args.refine_iters,
                                              n_streams=args.streams, group=args.group, confidence=confidence)
            else:
                res = sequence.register_images(model, images, Kcam, itr=args.itr, reperr=2.0, seed0=(s << 20) + lo,
                                               refine_iters=args.refine_iters, n_streams=args.streams,
                                               confidence=confidence)
            poses, status = sequence.stack_poses(res)
            n_eval = torch.cat([r.n_eval for r in res])
            ev = torch.cuda.Event()
            ev.record(reg_streams[s & 1])
        return poses, status, n_eval, ev, (res[0].idx, res[0].logp)

    cur = {"model": model, "Q": Q_all}      # what register() runs on (the f32 step below swaps both)
    reg_streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    tail_stream = torch.cuda.Stream(device=dev, priority=-1)

    def owner_of(image: int) -> int:
        return next(r for r in range(world) if shard.block_range(n_total, r, world)[0] <= image < shard.block_range(n_total, r, world)[1])

    def verify(poses, status, n_eval, ev, k1_first):
        """Every rank: pose all-gather + its share of the verification — `--verify pick`: the consecutive pairs it
        owns, then ONE all-reduce(MIN) over the f64 table (verfication.py:61-108); `--verify vote`: its rows of the
        n x n ADD-S vote, then the row-sum all-gather (choosePose.py:121-151 -> icp.py:37-39).  The rank that OWNS the
        chosen image runs ICP + final Chamfer for it (a14-a15): no rank is the slow one of every step.  Runs on its
        own stream and, pipelined, in a worker thread (current device and stream are thread-local; this thread
        issues the step's collectives, the main thread issues none inside the timed loop)."""
        torch.cuda.set_device(dev)
        if args.ablate == "noverify":
            ev.synchronize()
            return {"ablate": "noverify", "registered_this_rank": int(status.sum().item()), "_k1_first": k1_first}
        with torch.cuda.stream(tail_stream):
            tail_stream.wait_event(ev)
            poses_all = shard.allgather_rows(poses, n_total)
            out = {}
            if args.verify == "vote":
                Pa = poses_all.reshape(-1, 3, 4)
                vst = {}
                best, top, err = sequence.vote_choose_image(cad_d, pts, R_gt, t_gt, Pa[:, :, :3], Pa[:, :, 3], diameter, stats=vst)
                out.update(picked_image=best, vote_top5=[int(v) for v in top[:5]], vote_row_sum=float(err.sum(1).max()) if len(err) else None,
                           vote_items_searched=vst.get("exact"), vote_items=vst.get("items"))
            else:
                best, ch, table = sequence.pick_by_chamfer_table(pts, poses_all, R_gt, t_gt, n_total)
                out.update(picked_pair=best, picked_image=best, pair_chamfer=ch, chamfer_table=table)
            st = status.cpu()
            out.update(_poses_local=poses, _status_local=status, _k1_first=k1_first)
            out.update(registered_this_rank=int(st.sum().item()), images_this_rank=int(st.numel()),
                       hypotheses_scored_mean=float(n_eval.float().mean().item()), icp_rank=owner_of(best),
                       poses_all=poses_all.cpu().numpy())
            if rank == out["icp_rank"]:
                pose = out["poses_all"][best].reshape(3, 4)
                src = (upper.astype(np.float64) @ R_gt[best].T + t_gt[best]).astype(np.float32)   # icp.py:68
                init = np.linalg.inv(np.vstack([pose, [0, 0, 0, 1]]))                               # icp.py:88-92
                T, fit, rmse = registration.icp_point_to_point(src, lower, 20, init, max_iter=args.icp_iters, spatial_order=False)
                out.update(final_chamfer=registration.final_chamfer(src, lower, T, cad), icp_fitness=fit,
                           icp_rmse=rmse, _icp_T=T, rot_err_rad=synth.rot_angle(pose[:, :3], R_gt[best]),
                           trans_err_mm=float(np.linalg.norm(pose[:, 3] - t_gt[best])))
        return out

    step_done: list[float] = []            # host time at which each pipelined step's verification returned (diagnostics)

    def run_steps(first: int, count: int, confidence: float):
        """`count` steps.  Pipelined (default): registration of batch s + 1 is enqueued as soon as batch
        s's registration is, and batch s's verification (all-gather, pick or vote, ICP, final Chamfer —
        VALU work and chains of small dependent launches) runs from a worker thread on a high-priority
        stream beside it; the main thread never runs more than one batch ahead.  Batches are
        independent and every step's work is finished before this returns.  --no-pipeline runs
        registration and verification strictly one after the other."""
        last = None
        if args.no_pipeline or count <= 1:
            for s in range(first, first + count):
                last = verify(*register(s, confidence))
            return last
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        pending = deque()
        with ThreadPoolExecutor(max_workers=1) as pool:      # one worker: the collectives keep their order
            for s in range(first, first + count):
                r = register(s, confidence)
                while len(pending) >= max(args.depth, 1):
                    last = pending.popleft().result()
                    step_done.append(time.perf_counter())
                pending.append(pool.submit(verify, *r))
            while pending:
                last = pending.popleft().result()
                step_done.append(time.perf_counter())
        return last

    def barrier():
        torch.cuda.synchronize()
        if torch.distributed.is_initialized():
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def timed(first: int, count: int, confidence: float):
        # Python's cyclic collector is paused over the timed steps (collected just before, re-enabled after): a generation-2 pass
        # in the thread that enqueues the next batch is a host pause of milliseconds that shows up as an idle GPU — with it
        # running, one repetition in three lost 1-3 % on one box (profiles/r05_host_gc_ab.txt).  No work is skipped; reference
        # counting frees everything the loop drops.  --host-gc leaves the collector on.
        import gc
        gc_was = gc.isenabled()
        if not args.host_gc:
            gc.collect()
            gc.disable()
        barrier()
        t0 = time.perf_counter()
        last = run_steps(first, count, confidence)
        barrier()
        dt_rank = time.perf_counter() - t0
        if gc_was:
            gc.enable()
        dts = [dt_rank]
        if world > 1:
            tt = torch.zeros(world, dtype=torch.float64, device=shard._coll_device())
            tt[rank] = dt_rank
            torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
            dts = [float(v) for v in tt.cpu()]
        return last, max(dts), dts

    run_steps(0, args.warmup, args.confidence)
    # K1 with the chip to itself (untimed region, rank 0): the in-step figure below shares the GPU with the
    # RANSAC chains and the previous batch's verification, this one is the kernel alone
    k1_alone_ms = k1_clock_mhz = k1_rechecked = k1_screen = None
    if args.full and rank == 0:
        g_rows = Q_all[:max(args.group, 1)].reshape(-1, D)
        dig = dict(rows_per_image=P) if sequence.EPILOGUE_DIGITS else {}      # the call the step makes
        ops.corr_argmax(g_rows, model.keys, log2_prescaled=model.log2_queries, screened=model.screened, **dig)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(2):
            ops.corr_argmax(g_rows, model.keys, log2_prescaled=model.log2_queries, screened=model.screened, **dig)
        e1.record()
        torch.cuda.synchronize()
        k1_alone_ms = e0.elapsed_time(e1) / 2
        k1_clock_mhz = ops.corr_clock_mhz()        # shader clock held under the kernel (s_memtime / s_memrealtime)
        k1_rechecked = ops.corr_recheck_count()
        if model.screened:
            redone, handed = ops.corr_screen_redone()
            items = (g_rows.shape[0] // 32) * ((N + 31) // 32)
            # the same rows through the unscreened log2-domain kernel, alone: what the screen is measured against
            ops.corr_argmax(g_rows, model.keys, log2_prescaled=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(2):
                ops.corr_argmax(g_rows, model.keys, log2_prescaled=True)
            e1.record()
            torch.cuda.synchronize()
            k1_screen = {"tile_items_fetched_and_redone_frac": redone / items, "query_blocks_handed_to_the_dense_kernel": handed,
                         "T_log2_units": 21 + int(np.ceil(np.log2(N))),
                         "unscreened_kernel_alone_ms_per_launch": e0.elapsed_time(e1) / 2,
                         "note": "ISR_DTYPE_BF16_LOG2_SCREENED: every tile through one FP6 matrix instruction twice (pass 0: the "
                                 "query's lower bound L_q; pass 1: the screen), bf16 logits only for tiles that can hold a piece "
                                 "within T of L_q; flop_per_launch stays the ALGORITHMIC 2 P N D"}
    # untimed region, rank 0: the brute-force NN rate at the Chamfer-pair shape and the exact-f32 K1 on one image
    nn_live = f32_exact = nn_vote = k2_live = None
    if args.full and rank == 0:
        nn_live = measure_nn(pts, dev)
        k2_live = measure_ransac(dev, pts, Kcam, M=int(0.8 * P), H=max(args.itr, 4096))
        if args.verify == "vote":
            nn_vote = measure_nn_vote(cad_d, pts, dev, items=min(4096, n_local * n_total))
        f32_exact = measure_k1_f32(Q_all[0], keys_f32, dev, args.k1 != "natural")
    # per-entry-point HIP events inside the timed steps feed the roofline / stage figures of --full only
    ops.enable_timing(args.full)
    step_done.clear()
    last, dt, dts = timed(args.warmup, args.steps, args.confidence)
    step_intervals_ms = [(b - a) * 1e3 for a, b in zip(step_done[:-1], step_done[1:])]
    timing = ops.drain_timing()
    ops.enable_timing(False)
    # the ICP result of the last step lives on the rank that owned the chosen image: bring it to rank 0
    if world > 1 and args.ablate != "noverify":
        vals = torch.zeros(21, dtype=torch.float64, device=shard._coll_device())
        if rank == last["icp_rank"]:
            vals[:] = torch.tensor([last["final_chamfer"], last["icp_fitness"], last["icp_rmse"], last["rot_err_rad"],
                                    last["trans_err_mm"], *np.asarray(last["_icp_T"]).reshape(16)], dtype=torch.float64)
        torch.distributed.broadcast(vals, src=last["icp_rank"])
        v = [float(x) for x in vals.cpu()]
        last.update(final_chamfer=v[0], icp_fitness=v[1], icp_rmse=v[2], rot_err_rad=v[3], trans_err_mm=v[4],
                    _icp_T=np.array(v[5:]).reshape(4, 4))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)
    # untimed tail, every rank: the reference's per-image acceptance bookkeeping (inference.py:299-320, the T-LESS branch:
    # ADD-S of the pose and of its rotation alone against 0.1 x diameter) for the last step's block, summed over ranks
    acceptance = None
    if args.full and args.ablate != "noverify":
        acc = sequence.acceptance_counts(cad_d, pts, R_gt[lo:hi], t_gt[lo:hi], last["_poses_local"], last["_status_local"],
                                         diameter, dataset="tless")
        fin = np.isfinite(acc["final_error"])
        cnt = torch.tensor([acc["workCT"], acc["rotWorkCT"], int(fin.sum()), n_local], dtype=torch.float64)
        err_sum = torch.tensor([float(acc["final_error"][fin].sum())], dtype=torch.float64)
        if world > 1:
            both = torch.cat([cnt, err_sum]).to(shard._coll_device())
            torch.distributed.all_reduce(both)
            cnt, err_sum = both[:4].cpu(), both[4:].cpu()
        acceptance = {"rule": "ADDS(modelVerts, gtR, gtT, R, T) < 0.1 * diameter (inference.py:300-312, T-LESS branch)",
                      "diameter_mm": float(diameter), "workCT": int(cnt[0]), "rotWorkCT": int(cnt[1]),
                      "registered": int(cnt[2]), "images": int(cnt[3]),
                      "mean_adds_mm_of_registered": float(err_sum[0] / max(float(cnt[2]), 1.0))}
    # second short timed loop (untimed for `value`): the same step with EVERY hypothesis scored (confidence 1), so the
    # line carries the cv2-default figure and the score-everything one side by side
    all_hyp = None
    if args.full and args.confidence < 1.0 and args.ablate != "noverify":
        k = max(2, min(4, args.steps))
        last_all, dt_all, _ = timed(args.warmup + args.steps, k, 1.0)
        all_hyp = {"value": n_total * k / dt_all, "unit": "images/s", "steps": k, "ms_per_step": dt_all / k * 1e3,
                   "ransac_confidence": 1.0, "hypotheses_scored_mean": last_all.get("hypotheses_scored_mean"),
                   "note": "same step, every one of the --itr hypotheses scored (round 1's rule); not `value`"}

    def final_of(last_x):
        """final Chamfer of an untimed extra step on every rank (it lives on the rank that owned the picked image)."""
        fc = last_x.get("final_chamfer")
        if world > 1:
            v = torch.tensor([fc if (fc is not None and rank == last_x["icp_rank"]) else 0.0], dtype=torch.float64, device=shard._coll_device())
            torch.distributed.broadcast(v, src=last_x["icp_rank"])
            fc = float(v.cpu()[0])
        return fc

    # UNTIMED: the same step at the reference's own precision (inference.py:142-149 is an f32 matmul): f32 keys, f32 queries,
    # K1 on the f16-plane route; a few steps, every rank (the step has collectives)
    f32_step = None
    if args.full and args.group > 1 and args.ablate != "noverify" and not args.no_f32_step:
        k = max(2, min(4, args.steps))
        cur["model"] = sequence.SequenceModel(keys=keys_f32, pts=pts)
        cur["Q"] = (Q_all.float() / (ops.LOG2E if args.k1 != "natural" else 1.0)).contiguous()
        run_steps(args.warmup + 2 * args.steps, 1, args.confidence)
        last32, dt32, _ = timed(args.warmup + 2 * args.steps + 1, k, args.confidence)
        f32_step = {"value": n_total * k / dt32, "unit": "images/s", "steps": k, "ms_per_step": dt32 / k * 1e3,
                    "dtype": "f32 descriptors (K1: f16 planes on the 16-bit matrix cores, exact f32-chain indices)",
                    "final_chamfer": final_of(last32), "registered_this_rank": last32.get("registered_this_rank"),
                    "note": "the same step on f32 keys and queries — the reference's precision; not `value`"}
        if rank == 0 and not args.no_parity_check:
            from oracle import cbind
            rows = cur["Q"][0][:: max(1, P // 1024)][:1024].contiguous()
            idx_dev, logp_dev = ops.corr_argmax(rows, keys_f32)
            o = cbind.corr_argmax_f32(rows.cpu().numpy(), keys_f32.cpu().numpy())
            f32_step["parity_check"] = {"k1_rows_checked": int(rows.shape[0]),
                                        "k1_idx_equal_rows": int((idx_dev.cpu().numpy() == o["idx"]).sum()),
                                        "k1_logp_max_abs": float(np.abs(logp_dev.cpu().numpy() - (o["maxlogit"].astype(np.float64) - o["lse"])).max()),
                                        "picked_image": last32.get("picked_image"), "rot_err_rad": last32.get("rot_err_rad"),
                                        "trans_err_mm": last32.get("trans_err_mm")}
        cur["model"], cur["Q"] = model, Q_all

    # UNTIMED: the step on SURVEY 8(d)'s first recipe, |k| = 8 — a softmax peaked beyond f32 resolution, where K1's FP6 screen
    # (ISR_DTYPE_BF16_LOG2_SCREENED) can skip — unscreened and screened on the same data.  (At the bench's |k| = 5 every term
    # of the sums counts and the screened dtype hands every block to the dense kernel: DESIGN.md section 4 K1d.)
    screened_step = None
    if (args.full and args.group > 1 and args.ablate != "noverify" and not args.no_screened_step and D == 64 and args.k1 != "natural"
            and args.object == "tless"):
        keys8 = make_model(dev, N, D, tau=8.0, obj=args.object)[0]
        Q8 = torch.empty_like(Q_all)
        for j, i in enumerate(range(lo, hi)):
            Q8[j] = make_image(dev, keys8, pts, Kcam, R_gt[i], t_gt[i], P, i, True)[0]
        k = max(2, min(4, args.steps))
        screened_step = {"descriptor_norm": 8.0, "note": "SURVEY 8(d)'s |k| = 8 data; not `value`"}
        for name, scr in (("unscreened", False), ("screened", True)):
            cur["model"] = sequence.SequenceModel(keys=keys8.bfloat16(), pts=pts, log2_queries=True, screened=scr)
            cur["Q"] = Q8
            base = args.warmup + 3 * args.steps + (8 if scr else 0)
            run_steps(base, 1, args.confidence)
            last8, dt8, _ = timed(base + 1, k, args.confidence)
            screened_step[name] = {"value": n_total * k / dt8, "unit": "images/s", "ms_per_step": dt8 / k * 1e3,
                                   "final_chamfer": final_of(last8), "registered_this_rank": last8.get("registered_this_rank"),
                                   "picked_image": last8.get("picked_image")}
            if rank == 0:
                g_rows = Q8[:max(args.group, 1)].reshape(-1, D)
                out8 = ops.corr_argmax(g_rows, cur["model"].keys, log2_prescaled=True, screened=scr)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(2):
                    ops.corr_argmax(g_rows, cur["model"].keys, log2_prescaled=True, screened=scr)
                e1.record()
                torch.cuda.synchronize()
                ms8 = e0.elapsed_time(e1) / 2
                screened_step[name]["k1_alone_ms_per_launch"] = ms8
                screened_step[name]["k1_alone_frac_of_bf16_peak"] = 2.0 * g_rows.shape[0] * N * D / (ms8 * 1e-3) / PEAK_BF16_MFMA
                if scr:
                    redone, handed = ops.corr_screen_redone()
                    screened_step[name]["tile_items_fetched_and_redone_frac"] = redone / ((g_rows.shape[0] // 32) * ((N + 31) // 32))
                    screened_step[name]["query_blocks_handed_to_the_dense_kernel"] = handed
                    screened_step["k1_idx_equal"] = bool(torch.equal(out8[0], idx8_ref))
                    screened_step["k1_logp_max_abs_diff"] = float((out8[1] - logp8_ref).abs().max())
                else:
                    idx8_ref, logp8_ref = out8
        cur["model"], cur["Q"] = model, Q_all
        del Q8

    if rank == 0:
        verification = ("consecutive-pair Chamfer pick (one f64 min-table all-reduce)" if args.verify == "pick" else
                        "n x n ADD-S vote, rows sharded (row-sum all-gather)")
        last_pub = {k: v for k, v in last.items() if k not in ("poses_all", "chamfer_table") and not k.startswith("_")}
        line = {
            "metric": "registered images/sec (T-LESS obj 1-like, synthetic) + final Chamfer error",
            "value": n_total * args.steps / dt, "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            # what torch.distributed itself reports (not the flags): a SCALE record shows the backend saw N ranks
            "dist": ({"initialized": True, "backend": torch.distributed.get_backend(),
                      "world_size": torch.distributed.get_world_size(), "rank": torch.distributed.get_rank()}
                     if torch.distributed.is_initialized() else {"initialized": False, "backend": None, "world_size": 1, "rank": 0}),
            "config": {"workload": (f"BASELINE configs[1]: {n_local} images/GPU, {args.width}x{args.height}x{D}-D bf16 "
                                    f"queries vs {N} keys; per image getCors + top-80% filter + PnP-RANSAC "
                                    f"(<= {args.itr} P3P hypotheses, adaptive at confidence {args.confidence}, 2 px); per step "
                                    f"{verification}, ICP + final Chamfer on the rank that owns the chosen image"),
                       "verification": args.verify,
                       "images_per_gpu": n_local, "P": P, "N": N, "D": D, "hypotheses": args.itr,
                       "ransac_confidence": args.confidence,
                       "hypotheses_scored_mean": last.get("hypotheses_scored_mean"),
                       "parallelism": f"image-sharded x{world}",
                       "host": "python thread enqueues; cyclic GC " + ("enabled" if args.host_gc else "paused over the timed steps (--host-gc: on)"),
                       "cut_first_histogram": "K1 epilogue (isr_corr_argmax_digits)" if sequence.EPILOGUE_DIGITS else "hist_kernel<21,11> (isr_select_top_batch)",
                       "step_overlap": ("none" if args.no_pipeline else
                                        "verification (all-gather, pick/vote, ICP, final Chamfer) of batch s "
                                        "overlaps the registration of batch s+1")},
            "final_chamfer": last.get("final_chamfer"), "last_step": last_pub,
            "object": args.object,
            "step_intervals_ms": {"what": "host time between consecutive steps' verification results on this rank (the last one includes the "
                                          "pipeline's drain)", "values": [round(v, 2) for v in step_intervals_ms]},
            "per_rank_ms_per_step": {"min": min(dts) / args.steps * 1e3, "max": max(dts) / args.steps * 1e3,
                                     "all": [d / args.steps * 1e3 for d in dts]},
        }
        if args.full:
            calls, ms, flop = timing.get("corr_argmax", (0, 0.0, 0.0))
            k1_ms = ms / max(calls, 1)
            k1 = flop / max(calls, 1) / (k1_ms * 1e-3) if calls else 0.0
            # HBM bytes per launch come from PMC counters, which cannot be read inside a timed run: a separate
            # rocprofv3 --pmc pass of this very command (tools/pmc_traffic.sh) writes profiles/k1_hbm_traffic.json
            traffic = traffic_src = None
            pmc = ROOT / "profiles" / "k1_hbm_traffic.json"
            if pmc.exists() and (P, N, D) == (307200, 20000, 64):   # measured for this configuration only
                rec = json.loads(pmc.read_text()).get("per_launch", {}).get(str(max(args.group, 1)))
                if rec:
                    traffic, traffic_src = rec["hbm_bytes"], "profiles/k1_hbm_traffic.json: " + rec.get("source", "rocprofv3 --pmc")
            ncalls, nms, pairs = timing.get("nn_batched", (0, 0.0, 0.0))
            line.update({
                "acceptance": acceptance,
                "ransac_all_hypotheses": all_hyp,
                "f32_step": f32_step,
                "screened_step": screened_step,
                "roofline": {"kernel": ({"screened": "corr_quant_fp6_kernel x2 + corr_fp6_lower_kernel + corr_fp6_sparse_kernel (the whole "
                                                     "isr_corr_argmax call; HIP events around it)",
                                         "log2": "corr_bf16_direct_kernel", "natural": "corr_bf16_kernel"}[args.k1])
                                       + " (K1 getCors: MFMA GEMM + online LSE + argmax)",
                             "screen": k1_screen,
                             "k1_domain": args.k1,
                             "bound": "mfma", "achieved": k1 * 1e-12, "peak": PEAK_BF16_MFMA * 1e-12,
                             "unit": "TFLOP/s", "frac": k1 / PEAK_BF16_MFMA, "traffic": traffic, "traffic_source": traffic_src,
                             "algorithmic_bytes": 2.0 * P * max(args.group, 1) * D + 2.0 * N * D + 8.0 * P * max(args.group, 1),
                             "ms_per_launch": k1_ms, "launches": calls,
                             "ms_per_launch_covers": ("HIP events on the K1 stream around the opening half of each call: corr_keynorm_kernel + "
                                                      "the chip-filling kernel (the closing kernels — fallback, finalize, recheck, merge — run on "
                                                      "the group's side stream: isr_corr_argmax_phase)" if sequence.K1_SPLIT_CLOSE and args.group > 1
                                                      else "HIP events on the K1 stream around the whole isr_corr_argmax call"),
                             "clock_mhz_under_kernel": k1_clock_mhz,
                             "frac_at_held_clock": (k1 / (PEAK_BF16_MFMA * k1_clock_mhz / 2400.0)) if k1_clock_mhz else None,
                             "clock_note": "peak is quoted at the 2400 MHz boost clock; frac_at_held_clock scales it to the clock "
                                           "one workgroup of the kernel measured (alone on the GPU, untimed region)",
                             "queries_decided_by_exact_recheck": k1_rechecked,
                             "alone": {"ms_per_launch": k1_alone_ms,
                                       "frac": (flop / max(calls, 1) / (k1_alone_ms * 1e-3) / PEAK_BF16_MFMA
                                                if calls and k1_alone_ms else None),
                                       "note": "same launch with nothing else on the GPU (incl. finalize), untimed region"},
                             "flop_per_launch": flop / max(calls, 1), "images_per_launch": max(args.group, 1),
                             "exp_per_s": flop / max(calls, 1) / (2.0 * D) / (k1_ms * 1e-3) if calls else 0.0,
                             "f32_exact": f32_exact},
                "roofline_nn": nn_live,
                "roofline_nn_vote": nn_vote,
                "roofline_ransac": k2_live,
                # K3 is no longer one kernel at one rate: single-item calls (ICP steps, final Chamfer) scan every
                # target (nn_search_kernel, VALU-bound), the batched Chamfer pick runs the block-cooperative grid
                # search, which evaluates only the candidates near each query cell.  Reported: the rate in
                # brute-force-EQUIVALENT pairs (B Nq Nt per call) — a throughput figure, not a roofline fraction.
                "nn_stage": {"kernels": "nn_search_kernel (brute force: ICP, final Chamfer, vote items) / nn_tile_search_kernel "
                                        "(block-cooperative grid: batched pick)",
                             "equivalent_pairs_per_s": pairs / (nms * 1e-3) if ncalls else 0.0, "calls": ncalls,
                             "ms_per_step": nms / args.steps,
                             "note": "brute-force rate measured live: roofline_nn; DESIGN.md section 4 (K3/K4)"},
                "stage_ms_per_step": {k: v[1] / args.steps for k, v in timing.items()},
            })
            if world == 1 and not args.no_estimate_pose:
                try:
                    line["estimate_pose"] = measure_estimate_pose(dev)
                except Exception as e:
                    line["estimate_pose"] = {"error": repr(e)}
                try:
                    line["reference_shape"] = measure_reference_shape(dev)
                except Exception as e:
                    line["reference_shape"] = {"error": repr(e)}
            if not args.no_parity_check and args.ablate != "noverify":
                try:
                    line["parity_check"] = parity_check(args, model, Q_all[0], keys, pts, last, R_gt, t_gt, upper, lower, cad)
                except Exception as e:  # the GPU line must survive a checker-side failure
                    line["parity_check"] = {"error": repr(e)}
            if world == 1 and not args.no_cpu_baseline:
                try:
                    line["cpu_baseline"] = cpu_baseline(args, keys, pts, images[0][0], images[0][1], Kcam, upper,
                                                        lower, cad, R_gt, t_gt)
                except Exception as e:  # the GPU line must survive a checker-side failure
                    line["cpu_baseline"] = {"value": None, "error": repr(e), "kind": "port"}
        print(json.dumps(line), flush=True)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
