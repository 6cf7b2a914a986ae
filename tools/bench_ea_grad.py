"""The emission-absorption march with a gradient (isr_ea_march forward, isr_ea_march_backward backward), forward plus backward,
timed with HIP events:
    python tools/bench_ea_grad.py [--out profiles/ea_grad.json] [--rounds 7] [--calls 20]
  * trainNerfFine.py's coarse pass, (1 200, 64, 3), and its fine pass, (1 200, 128, 3);
  * the grid shape, (50 176, 256, 3): a 224 x 224 image at 256 samples a ray.
Each against
  * pren.py:362-367 written in torch (tests/ea_grad_ref.pren_march) under autograd on the same device and inputs;
  * the launch floor: as many one-element fills as the package's route launches kernels (two: the march and its backward),
    what those launches cost whatever they compute;
  * the byte floor: features read once and dfeatures written once at 6.3 TB/s.
A round is `calls` forward+backward calls between two events, after one warm-up call of every route; the record holds the
median, the fastest and the slowest round per call.  Also recorded: the peak memory of one call beyond what is allocated
before it (inputs and upstream gradients; the outputs and input gradients are part of the peak for both routes), and whether
two calls of each route give identical bytes.  No threshold: the record is the measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops, rays
from tests import ea_grad_ref as ref

HBM_BYTES_PER_S = 6.3e12
SHAPES = (("trainNerfFine.py's coarse pass", 1200, 64, 3), ("trainNerfFine.py's fine pass", 1200, 128, 3),
          ("the grid: 224 x 224 rays at 256 samples", 50176, 256, 3))


def timed(fn, rounds, calls):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "rounds": rounds,
            "calls_per_round": calls}


def routes(dens, feat, wi, ww):
    def package():
        dens.grad = feat.grad = None
        images, weights = rays.ea_march(dens[..., None], feat)
        torch.autograd.backward((images, weights), (wi, ww))
        return dens.grad, feat.grad

    def reference():
        dens.grad = feat.grad = None
        images, weights = ref.pren_march(dens, feat)
        torch.autograd.backward((images, weights), (wi, ww))
        return dens.grad, feat.grad

    return package, reference


def repeats(fn):
    a = [g.clone() for g in fn()]
    b = fn()
    return all(bool(torch.equal(x.view(torch.int32), y.view(torch.int32))) for x, y in zip(a, b))


def peak_beyond(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def case(name, N, P, F, dev, rounds, calls):
    rng = np.random.default_rng(1)
    t = lambda a: torch.from_numpy(a).to(dev)
    dens = t(ref.densities(rng, "sharp", N, P)).requires_grad_(True)
    feat = t(rng.uniform(0, 1, (N, P, F)).astype(np.float32)).requires_grad_(True)
    wi, ww = t(rng.standard_normal((N, F + 1)).astype(np.float32)), t(rng.standard_normal((N, P)).astype(np.float32))
    package, reference = routes(dens, feat, wi, ww)
    ours, theirs = [g.clone() for g in package()], reference()
    rec = {"case": name, "N": N, "P": P, "F": F, "rays_per_workgroup": ops.ea_grad_rays_per_group(P), "package_kernel_launches": 2,
           "largest_difference_from_torch": {"ddensities": float((ours[0] - theirs[0]).abs().max()),
                                             "dfeatures": float((ours[1] - theirs[1]).abs().max())},
           "torch_gradient_finite": bool(torch.isfinite(theirs[0]).all() and torch.isfinite(theirs[1]).all())}
    one = torch.empty(1, dtype=torch.int32, device=dev)
    rec["package_events"] = timed(package, rounds, calls)
    rec["torch_events"] = timed(reference, rounds, calls)
    rec["launch_floor_2_fills_events"] = timed(lambda: [one.fill_(1) for _ in range(2)], rounds, calls)
    rec["package_events_again"] = timed(package, rounds, calls)
    rec["byte_floor_ms"] = round(2 * 4 * N * P * F / HBM_BYTES_PER_S * 1e3, 5)
    ms = rec["package_events"]["median_ms"]
    rec["torch_over_package"] = round(rec["torch_events"]["median_ms"] / ms, 3)
    rec["package_over_launch_floor"] = round(ms / rec["launch_floor_2_fills_events"]["median_ms"], 2)
    rec["package_over_byte_floor"] = round(ms / rec["byte_floor_ms"], 2)
    rec["package_peak_bytes_beyond_inputs"] = peak_beyond(package)
    rec["torch_peak_bytes_beyond_inputs"] = peak_beyond(reference)
    rec["outputs_and_gradients_bytes"] = 4 * (N * (F + 1) + N * P + N * P + N * P * F)
    rec["package_two_calls_identical_bytes"] = repeats(package)
    rec["torch_two_calls_identical_bytes"] = repeats(reference)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    rows = []
    for name, N, P, F in SHAPES:
        rows.append(case(name, N, P, F, dev, a.rounds, a.calls))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "rays.ea_march(densities, features) and the backward of (images, weights) against pren.py:362-367 in torch "
                               "under autograd on the same device and inputs, the launch floor (one-element fills, one per kernel "
                               "launch of a route) and the byte floor (features read once, dfeatures written once, 6.3 TB/s).  HIP "
                               "events around `calls_per_round` forward+backward calls, per call; one process; the repeat-to-repeat "
                               "spread is min_ms .. max_ms and package_events_again",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "the forward and the backward kernels apart; the kernels torch's route launches, and their count; hardware "
                                       "counters; F other than 3; the step inside "
                                       "trainNerfFine.py (its fields are torch modules)",
                       "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
