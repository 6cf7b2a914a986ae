"""Farthest-point sampling on the device (isr_fps_sample: one launch per step) — a record, not a gate:
    python tools/bench_fps.py [--out profiles/fps_step.json] [--reps 5] [--shapes 729600x80000,80000x20000]
Per (M, K), one cloud of M points drawn in a unit-extent volume:
  * the whole call between HIP events, median of `reps` runs after a warm-up, and microseconds per step (time / (K - 1));
  * the floor in the same run: K back-to-back launches of an empty kernel on the same stream (isr_fps_launch_floor), so a
    step reads as "launch floor + x";
  * the comparator: isr_fps_sample_host (one thread) at the same M with K = 2 000, scaled linearly to K (the cost per step
    is constant) and marked extrapolated; over that prefix the device indices must equal the host's at full M (the first
    2 000 of a longer sequence are the sequence of K = 2 000);
  * the shader clock read from the driver before and after (the one marked current in pp_dpm_sclk), where it is readable."""
import argparse, glob, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops

HOST_K = 2000


def sclk_mhz():
    out = []
    for p in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            cur = [ln for ln in open(p).read().splitlines() if ln.rstrip().endswith("*")]
            out.append(cur[0].split()[1] if cur else None)
        except OSError:
            out.append(None)
    return out or "not readable"


def timed(fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="729600x80000,80000x20000")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    L = _capi.lib()
    stream = lambda: _capi.current_stream(dev)
    rows = []
    for shape in a.shapes.split(","):
        M, K = (int(v) for v in shape.split("x"))
        pts = np.random.default_rng(M).uniform(-0.5, 0.5, (M, 3)).astype(np.float32)
        d = torch.from_numpy(pts).to(dev)
        clock0 = sclk_mhz()
        idx = ops.fps_sample(d, K)                                       # warm-up, and the indices that are compared
        _capi.check(L.isr_fps_launch_floor(K, stream()), "isr_fps_launch_floor")
        torch.cuda.synchronize()
        dev_t = timed(lambda: ops.fps_sample(d, K), a.reps)
        floor_t = timed(lambda: _capi.check(L.isr_fps_launch_floor(K, stream()), "isr_fps_launch_floor"), a.reps)
        clock1 = sclk_mhz()
        hk = min(HOST_K, K)
        t0 = time.perf_counter()
        want = ops.fps_sample_host(pts, hk)[0]
        host_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(idx[:hk].cpu().numpy(), want), f"device and host indices differ over the first {hk} at M={M}"
        host_full = host_ms * (K - 1) / max(hk - 1, 1)
        row = {"M": M, "K": K, "device_call_events": dev_t, "device_us_per_step": round(dev_t["median_ms"] * 1e3 / (K - 1), 3),
               "empty_kernel_launches_events": floor_t, "floor_us_per_launch": round(floor_t["median_ms"] * 1e3 / K, 3),
               "step_over_floor_us": round((dev_t["median_ms"] - floor_t["median_ms"]) * 1e3 / (K - 1), 3),
               "host_one_thread": {"K": hk, "ms": round(host_ms, 1), "us_per_step": round(host_ms * 1e3 / max(hk - 1, 1), 2),
                                   "ms_at_K": round(host_full, 1), "extrapolated": hk < K},
               "host_over_device": round(host_full / dev_t["median_ms"], 2),
               "device_indices_equal_host_over_prefix": hk, "sclk_before": clock0, "sclk_after": clock1}
        print(json.dumps(row), flush=True)
        rows.append(row)
    doc = {"what": "isr_fps_sample (one launch per step, HIP events around the whole call) against the same number of empty-kernel "
                   "launches and against isr_fps_sample_host on one thread (K = 2000, scaled linearly to K)",
           "device": torch.cuda.get_device_name(0), "shapes": rows}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
