"""rays.sample_images_at_mc_locs with a gradient (isr_sample_nearest forward, isr_sample_nearest_backward backward), forward
plus backward, timed with HIP events:
    python tools/bench_sample_grad.py [--out profiles/sample_grad.json] [--rounds 7] [--calls 20]
  * run A, trainPose.py's shape: 16 images of 224 x 224 x 12, 1 024 Monte-Carlo rays each (the LDS sort);
  * run B, the full grid: 1 image of 224 x 224 x 12, 50 176 rays, each on its own pixel (the radix sort, two passes).
Each against
  * torch's grid_sample(mode='nearest', align_corners=True) under autograd on the same device and inputs (one fill and one
    kernel of float atomics);
  * the launch floor: as many one-element fills as the package's route launches kernels (the forward, the fill, the sort's
    and the sum), what those launches cost whatever they compute;
  * the byte floor: dimages written once and dout read once at 6.3 TB/s.
A round is `calls` forward+backward calls between two events, after one warm-up call of every route; the record holds the
median, the fastest and the slowest round per call.  The record also says whether two calls of each route give identical
bytes, on inputs with collisions (run A's, and run A's rays folded onto a 16 x 16 image).  No threshold: the record is the
measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops, rays
from tests import rays_ref, sample_grad_ref as ref

HBM_BYTES_PER_S = 6.3e12


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


def routes(feat, xys, up):
    B, n = xys.shape[:2]

    def package():
        feat.grad = None
        rays.sample_images_at_mc_locs(feat, xys).backward(up)
        return feat.grad

    def reference():
        feat.grad = None
        out = torch.nn.functional.grid_sample(feat.permute(0, 3, 1, 2), -xys.view(B, -1, 1, 2), align_corners=True, mode="nearest")
        out.permute(0, 2, 3, 1).view(B, n, -1).backward(up)
        return feat.grad

    return package, reference


def repeats(fn):
    a = fn().clone()
    b = fn().clone()
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def case(name, B, H, W, C, xys_h, dev, rounds, calls):
    rng = np.random.default_rng(1)
    n = xys_h.shape[1]
    feat = torch.from_numpy(rng.standard_normal((B, H, W, C)).astype(np.float32)).to(dev).requires_grad_(True)
    xys = torch.from_numpy(xys_h).to(dev)
    up = torch.from_numpy(rng.standard_normal((B, n, C)).astype(np.float32)).to(dev)
    package, reference = routes(feat, xys, up)
    _, _, m = ref.sums_f64(np.zeros((B, n, 1), np.float32), xys_h, H, W)
    diff = float((package().clone() - reference()).abs().max())
    geo = ops.sample_grad_geometry()
    passes = -(-(H * W).bit_length() // geo["digit_bits"])
    launches = 1 + 2 + (1 if n <= geo["lds_rays"] else 1 + 3 * passes)
    one = torch.empty(1, dtype=torch.int32, device=dev)
    rec = {"case": name, "B": B, "H": H, "W": W, "C": C, "n": n, "sort": "LDS" if n <= geo["lds_rays"] else f"radix, {passes} passes",
           "kernel_launches": launches, "rays_on_the_fullest_pixel": int(m.max()), "pixels_hit_more_than_once": int((m > 1).sum()),
           "largest_difference_from_torch": diff}
    rec["package_events"] = timed(package, rounds, calls)
    rec["torch_events"] = timed(reference, rounds, calls)
    rec["launch_floor_fills_events"] = timed(lambda: [one.fill_(1) for _ in range(launches)], rounds, calls)
    rec["package_events_again"] = timed(package, rounds, calls)
    nbytes = 4 * (B * H * W * C + B * n * C)
    rec["byte_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 5)
    rec["workspace_bytes"] = int(ops.lib().isr_sample_grad_workspace_bytes(B, H, W, n))
    ms = rec["package_events"]["median_ms"]
    rec["torch_over_package"] = round(rec["torch_events"]["median_ms"] / ms, 3)
    rec["package_over_launch_floor"] = round(ms / rec["launch_floor_fills_events"]["median_ms"], 2)
    rec["package_over_byte_floor"] = round(ms / rec["byte_floor_ms"], 2)
    rec["package_two_calls_identical_bytes"] = repeats(package)
    rec["torch_two_calls_identical_bytes"] = repeats(reference)
    return rec


def folded(xys_h, dev):
    """Run A's rays on a 16 x 16 x 12 image: 4 rays a pixel on average, so torch's atomics meet in every order."""
    rng = np.random.default_rng(3)
    B, n = xys_h.shape[:2]
    feat = torch.from_numpy(rng.standard_normal((B, 16, 16, 12)).astype(np.float32)).to(dev).requires_grad_(True)
    up = torch.from_numpy(rng.standard_normal((B, n, 12)).astype(np.float32)).to(dev)
    package, reference = routes(feat, torch.from_numpy(xys_h).to(dev), up)
    return {"what": "two calls on 16 images of 16 x 16 x 12 and 1 024 rays each: identical bytes?",
            "package": all(repeats(package) for _ in range(5)), "torch": all(repeats(reference) for _ in range(5))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    mc = np.random.default_rng(0).uniform(-1, 1, (16, 1024, 2)).astype(np.float32)
    rows = [case("A: trainPose.py's step, 16 images of 224 x 224 x 12, 1 024 rays each", 16, 224, 224, 12, mc, dev, a.rounds, a.calls),
            case("B: the full grid, 1 image of 224 x 224 x 12, 50 176 rays, each on its own pixel", 1, 224, 224, 12,
                 rays_ref.grid_xys(224, 224).reshape(1, -1, 2), dev, a.rounds, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    rep = folded(mc, dev)
    print(json.dumps(rep), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "rays.sample_images_at_mc_locs(feat, xys).backward(upstream) against torch's grid_sample(mode='nearest', "
                               "align_corners=True) under autograd on the same device and inputs, the launch floor (one-element fills, "
                               "one per kernel launch of the package's route) and the byte floor (dimages written once, dout read once, "
                               "6.3 TB/s).  HIP events around `calls_per_round` forward+backward calls, per call; one process; the "
                               "repeat-to-repeat spread is min_ms .. max_ms and package_events_again",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "the kernels apart (fill, sort, digit passes, sum); hardware counters; shapes other than the two; "
                                       "a long segment (thousands of rays on one pixel), which the serial chain makes slow on purpose; "
                                       "the step inside trainPose.py (its UNet is a torch module)",
                       "cases": rows, "collisions": rep}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
