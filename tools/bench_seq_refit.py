"""The sequence-level pose (ops.seq_refit) against the same iteratively reweighted solve composed from torch ops, in one process:
    python tools/bench_seq_refit.py [--out profiles/seq_refit.json] [--reps 7]
Scenes (tests/seq_refit_ref.scene): n = 1 280 and n = 64 frames, cap = 5 625 slots of which 4 500 are real, 0.5 px noise, 25 %
uniform outliers, a start 0.9 to 4.7 degrees and 3 to 8 mm off; Tukey k = 6, max_iter 30, the default tolerances.
Yardsticks, all in the same run: the torch composition (f64, the same rows, weights, sums by torch.sum, torch.linalg.solve,
the stop rule read on the host once per pass, as a torch user would write it); the launch floor (3 (max_iter + 1) empty
launches); the byte floor (20 bytes per real slot per executed pass at the device-to-device copy rate measured here).
Method: a warm-up round of each, then `reps` alternating rounds, host clock around work that ends in a synchronise: median
and min-max; the clocks are noted beside the numbers.  Also recorded: whether two calls give identical bytes, the passes and
the final error of both."""
import argparse, json, os, statistics, subprocess, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
from tests import seq_refit_ref as sr

K_TUKEY, MAX_ITER, TOL_R, TOL_T = 6.0, 30, 1e-10, 1e-8


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "rounds": len(ms)}


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l][:1]
    except Exception as e:            # the clock is a note beside the numbers, not a measurement
        return [f"not read: {e}"]


def torch_solve(p3d, p2d, counts, K, G, Y0):
    """The rule composed from torch ops in f64 on the device -> (Y, passes)."""
    n, cap = p3d.shape[:2]
    p, u = p3d.double(), p2d.double()
    Km, Gm = K.reshape(n, 3, 3), G.reshape(n, 3, 4)
    R, t = Gm[:, :, :3], Gm[:, :, 3]
    real = torch.arange(cap, device=p.device)[None, :] < counts[:, None]
    Y = Y0.clone()
    for it in range(MAX_ITER + 1):
        q = p @ Y[:3, :3].T + Y[:3, 3]
        c = torch.einsum("nab,nmb->nma", R, q) + t[:, None, :]
        h = torch.einsum("nab,nmb->nma", Km, c)
        pr = h[..., :2] / h[..., 2:3]
        r = pr - u
        rr = (r * r).sum(-1)
        a = rr.sqrt()
        w = torch.where(a <= K_TUKEY, (1 - (a / K_TUKEY) ** 2) ** 2, torch.zeros_like(a))
        ok = real & (c[..., 2] > 0) & torch.isfinite(rr) & (w > 0)
        w = torch.where(ok, w, torch.zeros_like(w))
        D = (Km[:, None, :2, :] - pr[..., None] * Km[:, None, 2:3, :]) / h[..., 2][..., None, None]
        g = torch.einsum("nmeb,nbc->nmec", D, R)
        J = torch.cat([torch.linalg.cross(q[:, :, None, :].expand_as(g), g), g], -1)
        J = torch.where(ok[..., None, None], J, torch.zeros_like(J))
        r = torch.where(ok[..., None], r, torch.zeros_like(r))
        wJ = w[..., None, None] * J
        A = torch.einsum("nmei,nmej->ij", wJ, J)
        b = torch.einsum("nmei,nme->i", wJ, r)
        x = torch.linalg.solve(A, -b)
        xh = x.cpu()                                         # the stop rule is read on the host, once per pass
        if float(xh[:3].abs().max()) < TOL_R and float(xh[3:].abs().max()) < TOL_T:
            return Y, it
        if it >= MAX_ITER:
            return Y, it
        qv = torch.cat([torch.ones(1, dtype=x.dtype, device=x.device), x[:3] / 2])
        qw, qx, qy, qz = (qv / qv.norm()).unbind()
        Rx = torch.stack([torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)]),
                          torch.stack([2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)]),
                          torch.stack([2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)])])
        dT = torch.eye(4, dtype=x.dtype, device=x.device)
        dT[:3, :3], dT[:3, 3] = Rx, x[3:]
        Y = dT @ Y
    return Y, MAX_ITER


def copy_rate(dev, nbytes=1 << 28, reps=5):
    a, b = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b.copy_(a)
    ms = [timed(lambda: b.copy_(a))[0] for _ in range(reps)]
    return 2 * nbytes / (statistics.median(ms) * 1e-3)       # bytes read + written per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="64,1280")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    L = _capi.lib()
    launches = 3 * (MAX_ITER + 1)
    floor = lambda: _capi.check(L.isr_fps_launch_floor(launches, torch.cuda.current_stream(dev).cuda_stream), "isr_fps_launch_floor")
    floor()
    rate = copy_rate(dev)
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        s = sr.scene(100 + n, n=n, m=4500, cap=5625)
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        p3d, p2d, counts, K, G, Y0 = (d(s[q]) for q in ("p3d", "p2d", "counts", "K", "G", "Y0"))

        def ours():
            st = torch.zeros(24, dtype=torch.float64, device=dev)
            st[:16] = Y0.reshape(16)
            return ops.seq_refit(p3d, p2d, counts, K, G, st, None, "tukey", K_TUKEY, MAX_ITER, TOL_R, TOL_T)

        composed = lambda: torch_solve(p3d, p2d, counts, K, G, Y0)
        r1, r2 = ours(), ours()
        torch.cuda.synchronize()
        identical = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(r1, r2))
        composed()
        t_ours, t_torch, t_floor = [], [], []
        for _ in range(a.reps):
            ms, ro = timed(ours)
            t_ours.append(ms)
            ms, rt = timed(composed)
            t_torch.append(ms)
            t_floor.append(timed(floor)[0])
        st = ro[0].cpu().numpy()
        passes = int(st[18]) + 1
        row = {"n": n, "cap": 5625, "real_rows_per_frame": 4500, "rows_counted_last_pass": int(st[19]), "launches_per_call": launches,
               "seq_refit": {**stats(t_ours), "passes": passes, "status": sr.STATUS[int(st[20])],
                             "final_error_deg_mm": [round(v, 5) for v in sr.pose_error(st[:16].reshape(4, 4), s["Y_true"])]},
               "torch_composition": {**stats(t_torch), "passes": rt[1] + 1,
                                     "final_error_deg_mm": [round(v, 5) for v in sr.pose_error(rt[0].cpu().numpy(), s["Y_true"])]},
               "start_error_deg_mm": [round(v, 4) for v in sr.pose_error(s["Y0"], s["Y_true"])],
               "launch_floor": stats(t_floor),
               "byte_floor_ms": round(20.0 * n * 4500 * passes / rate * 1e3, 4),
               "two_calls_identical_bytes": bool(identical)}
        row["torch_over_seq_refit"] = round(row["torch_composition"]["median_ms"] / row["seq_refit"]["median_ms"], 2)
        row["seq_refit_over_launch_floor"] = round(row["seq_refit"]["median_ms"] / row["launch_floor"]["median_ms"], 2)
        row["seq_refit_over_byte_floor"] = round(row["seq_refit"]["median_ms"] / row["byte_floor_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = {"what": "ops.seq_refit (Tukey, k = 6 px) vs the same solve composed from torch ops, same process, alternating rounds, "
                   "host clock; synthetic scenes",
           "device": torch.cuda.get_device_name(0), "clocks": sclk(), "max_iter": MAX_ITER, "tol": [TOL_R, TOL_T],
           "copy_rate_bytes_per_s": round(rate), "byte_floor": "20 bytes per real slot per executed pass at copy_rate",
           "launch_floor": f"{launches} empty launches (isr_fps_launch_floor)", "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
