"""Batched multi-start ICP against the loop of single calls, in one process:
    python tools/bench_icp_batch.py [--out profiles/icp_batch_vs_loop.json] [--reps 7] [--single-only]
For k in {1, 8, 50} starts and clouds of (5 000, 5 000) and (20 000, 20 000) points: registration.icp_point_to_point_batch
against k registration.icp_point_to_point calls (both from host arrays to host results, threshold 20, Open3D defaults),
the two alternating, `reps` timed rounds after a warm-up round of each; medians and the min-max spread, host clock around
work that ends in the device->host copy of the results.  The starts climb from 0.02 degrees to 60 degrees off the true
pose (and one 300 mm off, which finds no correspondence), so the items stop at different iterations.  Results are checked
bit for bit against each other while timing.  --single-only times the single call alone (comparing two builds of the
library: ISR_HIP_LIB selects the other one)."""
import argparse, json, os, statistics, subprocess, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import registration, synth

LADDER = [(0.02, 0.1), (3, 3), (25, 10), (0.5, 0.5), (3, 300), (10, 5), (60, 3), (1, 1)]


def problem(N, k, seed=20240):
    rng = np.random.default_rng(seed + N)
    cloud = synth.tless_like(rng, 4 * N)
    upper, lower = synth.split_halves(rng, cloud, N)
    Rg, tg = synth.random_poses(rng, k)
    srcs, inits = [], []
    for i in range(k):
        a, d = LADDER[i % len(LADDER)]
        Rp, tp = synth.perturb_pose(rng, Rg[i], tg[i], a * (1 + 0.1 * (i // len(LADDER))), d)
        srcs.append((upper.astype(np.float64) @ Rg[i].T + tg[i]).astype(np.float32))
        inits.append(np.linalg.inv(np.vstack([np.hstack([Rp, tp[:, None]]), [0, 0, 0, 1]])))
    return np.stack(srcs), lower, np.stack(inits)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "rounds": len(ms)}


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return [l.strip() for l in out.splitlines() if "sclk" in l][:1]
    except Exception as e:            # the clock is a note beside the numbers, not a measurement
        return [f"not read: {e}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--single-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.cuda.get_device_name(0)
    rows = []
    for N in (5000, 20000):
        for k in ((1,) if a.single_only else (1, 8, 50)):
            srcs, tgt, inits = problem(N, k)
            s_d, t_d = torch.from_numpy(srcs).cuda(), torch.from_numpy(tgt).cuda()      # clouds resident, as in the pipeline
            loop = lambda: [registration.icp_point_to_point(s_d[i], t_d, 20, inits[i]) for i in range(k)]
            batch = lambda: registration.icp_point_to_point_batch(s_d, t_d, 20, inits)
            loop()
            t_loop, t_batch = [], []
            if not a.single_only:
                batch()
            for _ in range(a.reps):
                ms, rl = timed(loop)
                t_loop.append(ms)
                if a.single_only:
                    continue
                ms, (T, fit, rmse, iters) = timed(batch)
                t_batch.append(ms)
                same = all(np.array_equal(T[i], rl[i][0]) and fit[i] == rl[i][1] and rmse[i] == rl[i][2] for i in range(k))
                assert same, "batch and loop disagree"
            row = {"Ns": N, "Nt": N, "k": k, "loop": stats(t_loop)}
            if not a.single_only:
                row["batch"] = stats(t_batch)
                row["loop_over_batch"] = round(row["loop"]["median_ms"] / row["batch"]["median_ms"], 2)
                row["iterations"] = sorted(set(int(x) for x in iters))
                row["bit_identical"] = True
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = {"what": "icp_point_to_point_batch vs a loop of icp_point_to_point calls, same process, alternating rounds",
           "device": dev, "clocks": sclk(), "library": os.environ.get("ISR_HIP_LIB", "in-tree"), "threshold": 20, "max_iter": 30,
           "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
