"""The useSurfEval branch (inference.py:324-366) on a block of crops at the reference's crop shape: (a) the per-image loop
(estimate_pose + best pose + refine_pose, one image after the other) against (b) sequence.estimate_and_refine (estimate_poses
for the block, refine_poses in lockstep: one batched objective launch per BFGS round).  Device-synchronised wall time after a
warm-up, the two arms alternated; both arms must give the same R2, T2, t_ref and fun.  Prints one JSON line.
--optimizer device: the block refines with refine_poses(optimizer="device") (scipy's BFGS as a state machine on the device,
one isr_refine_bfgs_batch call); its t_ref and fun then agree with the per-image scipy loop to rounding, not bit for bit,
and the record gives the largest differences and the items' BFGS statuses.

    python tools/bench_surf_eval.py [--B 32] [--m 20000] [--reps 3] [--optimizer scipy|device] [--out profiles/<name>.json]

The renderer and the feature field are stand-ins (a vectorised point z-buffer, a fixed sinusoidal field), as in the tests:
the reference's moderngl renderer and SIREN are not part of this package."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from imagesequenceregistrationfor6dposeestimationlabeling_amd import pose_est_surf, pose_refine, sequence, synth  # noqa: E402


class Obj:
    scale, diameter = 60.0, 120.0
    offset = np.zeros(3)


class Renderer:
    """(res,res,4) object coordinates / scale + mask of the nearest point per pixel (front-facing points only)."""
    def __init__(self, pts, nrm, res):
        self.pts, self.nrm, self.res = pts.astype(np.float64), nrm, res

    def render(self, obj_idx, K, R, t):
        R, t = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
        cam = self.pts @ R.T + t
        uv = cam @ np.asarray(K, np.float64).T
        uv = uv[:, :2] / uv[:, 2:]
        ui, vi = np.rint(uv[:, 0]).astype(int), np.rint(uv[:, 1]).astype(int)
        ok = np.nonzero((((self.nrm @ R.T) * cam).sum(1) < 0) & (ui >= 0) & (ui < self.res) & (vi >= 0) & (vi < self.res))[0]
        ok = ok[np.argsort(-cam[ok, 2], kind="stable")]
        img = np.zeros((self.res, self.res, 4), np.float32)
        img[vi[ok], ui[ok], :3] = self.pts[ok] / Obj.scale
        img[vi[ok], ui[ok], 3] = 1.0
        return img


class Field:
    def __init__(self, W):
        self.W = W

    def batched_customForward(self, x):
        f = torch.sin(x @ self.W.to(x.device))
        return torch.cat([f, torch.ones(len(x), 1, device=x.device)], dim=-1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--r", type=int, default=224)
    ap.add_argument("--e", type=int, default=12)
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--n-samples-denom", type=int, default=10960)
    ap.add_argument("--max-pose-evaluations", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--optimizer", choices=["scipy", "device"], default="scipy")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = synth.crop_block(a.B, 7, a.r, a.e, a.m)
    B = a.B
    rng = np.random.default_rng(3)
    field = Field(torch.from_numpy(rng.normal(0, 2.0, (3, a.e)).astype(np.float32)))
    rend = Renderer(s["pts"], s["normals"], a.r)
    ml, q = torch.from_numpy(s["mask_lgts"]).to(dev), torch.from_numpy(s["query"]).to(dev)
    pts, keys = torch.from_numpy(s["pts"]).to(dev), torch.from_numpy(s["keys"]).to(dev)
    nrm = torch.from_numpy(s["normals"]).to(dev)
    keys_verts = field.batched_customForward(torch.from_numpy(s["pts"] * 1.8 / Obj.diameter).to(dev))[:, :a.e].float()
    verts = s["pts"][::10]
    est_kw = dict(max_pose_evaluations=a.max_pose_evaluations)
    ref_kw = dict(n_samples_denom=a.n_samples_denom)

    def per_image():
        t_est = t_ref = 0.0
        rows, n_eval = [], []
        made = []
        base = pose_refine.RefineObjective

        class Counting(base):
            def __init__(self, *x, **k):
                super().__init__(*x, **k)
                made.append(self)
        pose_refine.RefineObjective = Counting
        try:
            for b in range(B):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                R, t, ps, ms = pose_est_surf.estimate_pose(ml[b], q[b], pts, nrm, keys, s["diameter"], s["K"].copy(), seed=b,
                                                           **est_kw)[:4]
                if len(ms) == 0:
                    torch.cuda.synchronize()
                    t_est += time.perf_counter() - t0
                    rows.append(None)
                    continue
                i = torch.argsort(ps)[-1]
                R2, T2 = R[i].cpu().numpy(), t[i].cpu().numpy()
                t1 = time.perf_counter()
                t_est += t1 - t0
                _, tr, fun = pose_refine.refine_pose(R2, T2, q[b], rend, 0, s["K"], Obj, field, keys_verts,
                                                     generator=torch.Generator(device=dev).manual_seed(b), **ref_kw)
                torch.cuda.synchronize()
                t_ref += time.perf_counter() - t1
                rows.append((R2, T2, tr, fun))
                n_eval.append(made[-1].n_launch)
        finally:
            pose_refine.RefineObjective = base
        return rows, t_est, t_ref, n_eval

    real_refine_poses = pose_refine.refine_poses

    def block():
        stats, t_refine = {}, []

        def timed_refine_poses(*x, **k):             # the block's refine share: refine_poses, device-synchronised
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r = real_refine_poses(*x, **k)
            torch.cuda.synchronize()
            t_refine.append(time.perf_counter() - t1)
            return r
        pose_refine.refine_poses = timed_refine_poses
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = sequence.estimate_and_refine(ml, q, pts, nrm, keys, s["diameter"], s["K"], rend, 0, Obj, field, keys_verts,
                                               verts, s["R"], s["t"], estimate_kw=est_kw,
                                               refine_kw=dict(ref_kw, stats=stats, optimizer=a.optimizer))
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
        finally:
            pose_refine.refine_poses = real_refine_poses
        return out, t, stats, sum(t_refine)

    per_image()                      # warm-up (kernels, workspaces, side streams)
    block()
    ta, tb, tbr = [], [], []
    for _ in range(a.reps):          # alternated arms
        rows, te, tr, n_eval = per_image()
        ta.append((te, tr))
        out, t, stats, t_r = block()
        tb.append(t)
        tbr.append(t_r)
    same = True
    dt_max = dfun_max = 0.0
    for b, r in enumerate(rows):
        if r is None:
            same &= not out["refined"][b]
            continue
        same &= bool(out["refined"][b] and np.array_equal(out["R2"][b], r[0]) and np.array_equal(out["T2"][b], r[1]))
        if a.optimizer == "scipy":
            same &= bool(np.array_equal(out["t_ref"][b], r[2]) and out["fun"][b] == r[3])
        else:                        # to rounding: the figures are recorded, a tolerance is the tests' business
            dt_max = max(dt_max, float(np.max(np.abs(np.asarray(out["t_ref"][b]) - np.asarray(r[2])))))
            dfun_max = max(dfun_max, abs(float(out["fun"][b]) - float(r[3])) / max(1.0, abs(float(r[3]))))
    med = lambda v: float(np.median(v))                                   # noqa: E731
    rec = dict(tool="bench_surf_eval", B=B, r=a.r, e=a.e, m=a.m, n_samples_denom=a.n_samples_denom,
               max_pose_evaluations=a.max_pose_evaluations, reps=a.reps, refined=int(out["refined"].sum()),
               per_image_estimate_ms_per_image=1e3 * med([x[0] for x in ta]) / B,
               per_image_refine_ms_per_image=1e3 * med([x[1] for x in ta]) / B,
               per_image_total_ms_per_image=1e3 * med([x[0] + x[1] for x in ta]) / B,
               block_total_ms_per_image=1e3 * med(tb) / B, block_refine_ms_per_image=1e3 * med(tbr) / B,
               optimizer=a.optimizer,
               lockstep_rounds=stats["rounds"], per_image_evaluations_sum=int(sum(n_eval)),
               per_image_evaluations_max=int(max(n_eval)) if n_eval else 0, batched_item_evaluations=int(sum(stats["n_eval"])),
               outputs_equal=bool(same), workCT=out["workCT"], refCT=out["refCT"], rotWorkCT=out["rotWorkCT"],
               device=torch.cuda.get_device_name(0))
    if a.optimizer == "device":
        rec.update(block_launches=stats["launches"], device_bfgs_nit_max=int(max(stats["nit"])),
                   device_bfgs_status=dict(zip(*[v.tolist() for v in np.unique(stats["status"], return_counts=True)])),
                   t_ref_max_abs_diff_mm=dt_max, fun_max_rel_diff=dfun_max)
        rec["device_bfgs_status"] = {str(k): int(v) for k, v in rec["device_bfgs_status"].items()}
    line = json.dumps(rec)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    if not same:
        sys.exit("the two arms disagree")


if __name__ == "__main__":
    main()
