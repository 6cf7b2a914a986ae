"""ops.pnp_ransac_batch with the Gauss-Newton refit as the final solve (final="refit", the default) against cv2's final solve,
EPnP over the winner's consensus set (final="epnp"), both on cv2's path otherwise (loop="sequential", inliers="ransac"), at
  (a) the bench step's shape: 64 images, M = 0.8 x 640 x 480 correspondences each, H = 500;
  (b) BASELINE configs[3]'s hypothesis count: H = 4096 at the same M (16 images);
  (c) the reference's crop shape: 128 crops of 75 x 75 (M = 2 000 here), H = 500.
Images carry outlier fractions from 0.2 to 0.85 and 0.5 px of pixel noise.  Device time per call from HIP events on the
launch stream after a warm-up, the arms alternated; the median rotation error against the synthetic ground truth per arm.
Prints one JSON line.

    python tools/bench_pnp_final.py [--reps 10] [--out profiles/<name>.json]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops, synth  # noqa: E402


def _case(dev, B, M, seed):
    rng = np.random.default_rng(seed)
    pts = synth.tless_like(rng, 4000)
    K = synth.camera()
    R, t = synth.random_poses(rng, B)
    p3 = np.empty((B, M, 3), np.float32)
    p2 = np.empty((B, M, 2), np.float32)
    fr = rng.uniform(0.2, 0.85, B)
    for b in range(B):
        p3[b], p2[b], _ = synth.pnp_case(rng, pts, K, R[b], t[b], M, 0.5, float(fr[b]))
    return (torch.from_numpy(p3).to(dev), torch.from_numpy(p2).to(dev), torch.full((B,), M, dtype=torch.int32, device=dev),
            K, R, t, fr)


def _measure(dev, name, B, M, H, reps, seed):
    p3, p2, M_dev, K, R, T, fr = _case(dev, B, M, seed)
    seeds = list(range(B))
    arms = {"refit": dict(loop="sequential", inliers="ransac"),
            "epnp": dict(loop="sequential", inliers="ransac", final="epnp")}
    out = {}
    for arm, kw in arms.items():                 # warm-up + the per-image record
        r = ops.pnp_ransac_batch(p3, p2, K, M_dev, H=H, reperr=2.0, seeds=seeds, **kw)
        torch.cuda.synchronize()
        ne = r.n_eval.cpu().numpy()
        pose = r.pose.cpu().numpy()
        err = [synth.rot_angle(pose[b, :, :3], R[b]) for b in range(B) if int(r.status[b].item())]
        tr = [float(np.linalg.norm(pose[b, :, 3] - T[b]) / np.linalg.norm(T[b])) for b in range(B) if int(r.status[b].item())]
        out[arm] = {"ms": [], "n_eval_mean": float(ne.mean()), "status_sum": int(r.status.sum().item()),
                    "rot_err_median_rad": float(np.median(err)) if err else None,
                    "rot_err_max_rad": float(np.max(err)) if err else None,
                    "t_rel_err_median": float(np.median(tr)) if tr else None}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for arm, kw in arms.items():
            e0.record()
            ops.pnp_ransac_batch(p3, p2, K, M_dev, H=H, reperr=2.0, seeds=seeds, **kw)
            e1.record()
            torch.cuda.synchronize()
            out[arm]["ms"].append(e0.elapsed_time(e1))
    for arm in arms:
        ms = sorted(out[arm].pop("ms"))
        out[arm].update(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], ms_per_image=ms[len(ms) // 2] / B)
    return {"shape": name, "B": B, "M": M, "H": H, "outlier_frac_range": [float(fr.min()), float(fr.max())],
            "epnp_over_refit": out["epnp"]["ms_median"] / out["refit"]["ms_median"], **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    M = int(0.8 * 640 * 480)
    rows = [_measure(dev, "bench step (64 images, H = 500)", 64, M, 500, args.reps, 1),
            _measure(dev, "configs[3] hypotheses (H = 4096)", 16, M, 4096, args.reps, 2),
            _measure(dev, "reference crops (128 x M = 2000, H = 500)", 128, 2000, 500, args.reps, 3)]
    rec = {"tool": "bench_pnp_final", "reps": args.reps, "timer": "HIP events around one pnp_ransac_batch call, median",
           "device": torch.cuda.get_device_name(dev), "rows": rows}
    line = json.dumps(rec)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
