"""ops.pnp_ransac_batch with the staged RANSAC loop (the default) against OpenCV's sequential loop (loop="sequential"), at
  (a) the bench step's shape: 64 images, M = 0.8 x 640 x 480 correspondences each, H = 500;
  (b) BASELINE configs[3]'s hypothesis count: H = 4096 at the same M (16 images);
  (c) the reference's crop shape: 128 crops of 75 x 75 (M = 2 000 here), H = 500.
Images carry outlier fractions from 0.2 to 0.85, so the loops stop at different points.  Device time per call from HIP
events on the launch stream after a warm-up, the two arms alternated.  Beside the times: the hypotheses each loop ran
(n_eval) and scored (the staged loop scores what it runs; the sequential loop scores whole stages up to the one holding its
stop).  The "*_norefit" arms (refine_iters = 0) time the loop without the Gauss-Newton refit, whose cost follows the
winner it starts from.  Prints one JSON line.

    python tools/bench_pnp_loop.py [--reps 10] [--out profiles/<name>.json]
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


def _scored(n_eval: int, H: int, stage0: int = 32) -> int:
    """Hypotheses the scoring stages [0, s), [s, 3 s), ... cover up to the one holding hypothesis n_eval - 1."""
    lo, ln = 0, stage0
    while lo + ln < min(n_eval, H):
        lo, ln = lo + ln, 2 * ln
    return min(H, lo + ln) if n_eval > 0 else 0


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
            K, R, fr)


def _measure(dev, name, B, M, H, reps, seed):
    p3, p2, M_dev, K, R, fr = _case(dev, B, M, seed)
    seeds = list(range(B))
    arms = {"staged": dict(), "sequential": dict(loop="sequential"),
            "staged_norefit": dict(refine_iters=0), "sequential_norefit": dict(loop="sequential", refine_iters=0)}
    out = {}
    for arm, kw in arms.items():                 # warm-up + the per-image record
        r = ops.pnp_ransac_batch(p3, p2, K, M_dev, H=H, reperr=2.0, seeds=seeds, **kw)
        torch.cuda.synchronize()
        ne = r.n_eval.cpu().numpy()
        pose = r.pose.cpu().numpy()
        err = [synth.rot_angle(pose[b, :, :3], R[b]) for b in range(B) if int(r.status[b].item())]
        out[arm] = {"ms": [], "n_eval_mean": float(ne.mean()), "n_eval_min": int(ne.min()), "n_eval_max": int(ne.max()),
                    "scored_sum": int(sum(ne) if arm.startswith("staged") else sum(_scored(int(n), H) for n in ne)),
                    "status_sum": int(r.status.sum().item()), "rot_err_median_rad": float(np.median(err)) if err else None}
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
            "sequential_over_staged": out["sequential"]["ms_median"] / out["staged"]["ms_median"],
            "sequential_over_staged_norefit": out["sequential_norefit"]["ms_median"] / out["staged_norefit"]["ms_median"], **out}


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
    rec = {"tool": "bench_pnp_loop", "reps": args.reps, "timer": "HIP events around one pnp_ransac_batch call, median",
           "device": torch.cuda.get_device_name(dev), "rows": rows}
    line = json.dumps(rec)
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
