"""The masked ray bundles of generateCors.py and genFeat.py on the device, timed with HIP events:
    python tools/bench_rays.py [--out profiles/rays.json] [--rounds 7] [--calls 20]
  * grid: NDCMultinomialRaysampler(224, 224, 256 points) for one camera under its silhouette (generateCors.py:136, :297-304);
  * mc:   MonteCarloRaysampler(30 rays, 128 points, strata) for 1 280 cameras under their silhouettes (genFeat.py:105, :162-189).
Each against the same steps written in torch on the same device (linspace / rand, the unprojection as a matmul, grid_sample,
torch.where, indexing — torch's random stream, so other rays: the work is the same, the values are not compared) and against
the launch floor: three one-element fills and one 4-byte read, which is what the three launches and the read of the count
cost whatever they compute.  A round is `calls` calls between two events, after one warm-up call of every route; the record
holds the median, the fastest and the slowest round per call.  The device bundle is compared with the host build before
timing.  No threshold: the record is the measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import rays


def cameras(B, dev, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)
    T = np.stack([rng.uniform(-0.1, 0.1, B), rng.uniform(-0.1, 0.1, B), rng.uniform(3, 4, B)], 1)
    f = rng.uniform(500, 700, (B, 1)).repeat(2, 1)
    p = 112 + rng.uniform(-5, 5, (B, 2))
    return rays.PerspectiveCameras(R, T, f, p, (224, 224), device=dev)


def silhouettes(B, dev, seed=1):
    """A disc per camera, a third of the image or so: (B, 224, 224) f32."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:224, 0:224]
    c = 112 + rng.uniform(-20, 20, (B, 2))
    r = rng.uniform(60, 80, B)
    m = (xx[None] - c[:, 0, None, None]) ** 2 + (yy[None] - c[:, 1, None, None]) ** 2 < r[:, None, None] ** 2
    return torch.from_numpy(m.astype(np.float32)).to(dev)


def torch_bundle(cams, xys, lengths, mask):
    """The reference's steps in torch: rays of xys (B, n, 2), then pren.py:231-235."""
    B, n = xys.shape[:2]
    K = cams.intrinsics
    c = torch.cat([(xys - K[:, None, 2:]) / K[:, None, :2], torch.ones(B, n, 1, device=xys.device)], -1)
    d = c @ cams.R.transpose(1, 2)
    o = (-cams.T[:, None] @ cams.R.transpose(1, 2)).expand(B, n, 3)
    sampled = torch.nn.functional.grid_sample(mask[:, None], -xys.view(B, -1, 1, 2), align_corners=True, mode="nearest")
    keep = torch.where(sampled.permute(0, 2, 3, 1).view(B, n, 1)[..., 0])
    return o[keep][None], d[keep][None], lengths[keep][None], xys[keep][None]


def torch_grid(cams, mask, P, lo, hi):
    dev = mask.device
    xs = torch.linspace(1 - 1 / 224, -1 + 1 / 224, 224, dtype=torch.float32, device=dev)
    Y, X = torch.meshgrid(xs, xs, indexing="ij")
    xys = torch.stack([X, Y], -1).view(1, -1, 2).expand(len(cams), -1, -1)
    lengths = torch.linspace(lo, hi, P, dtype=torch.float32, device=dev).expand(len(cams), 224 * 224, P)
    return torch_bundle(cams, xys, lengths, mask)


def torch_mc(cams, mask, n, P, lo, hi):
    dev = mask.device
    B = len(cams)
    xys = torch.rand(B, n, 2, device=dev) * 2 - 1
    l = torch.linspace(lo, hi, P, dtype=torch.float32, device=dev).expand(B, n, P)
    mids = 0.5 * (l[..., 1:] + l[..., :-1])
    upper, lower = torch.cat([mids, l[..., -1:]], -1), torch.cat([l[..., :1], mids], -1)
    return torch_bundle(cams, xys, lower + (upper - lower) * torch.rand_like(lower), mask)


def launch_floor(dev):
    a = torch.empty(1, dtype=torch.int32, device=dev)
    def run():
        a.fill_(1)
        a.fill_(2)
        a.fill_(3)
        return int(a.cpu()[0])
    return run


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


def same_as_host(sampler, cams, mask):
    got = sampler(cams, mask=mask)
    want = sampler(cams, mask=mask.cpu(), host=True)
    return all(g.shape == w.shape and torch.equal(g.cpu().view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want)), got


def case(name, sampler, cams, mask, other, rounds, calls):
    same, bundle = same_as_host(sampler, cams, mask)
    M, P = bundle.lengths.shape[1:]
    rec = {"case": name, "cameras": len(cams), "candidate_rays": int(len(cams) * sampler.spec.rays_per_camera), "kept_rays": int(M), "P": int(P),
           "bytes_written": int(M) * (8 * 4 + 4 * int(P)) + int(M) * 4, "device_bundle_equals_host_build": bool(same),
           "kept_rays_torch": int(other()[0].shape[1])}
    # alternate the routes, so that a busy neighbour on the machine meets all of them
    rec["rays_py_events"] = timed(lambda: sampler(cams, mask=mask), rounds, calls)
    rec["torch_events"] = timed(other, rounds, calls)
    rec["launch_floor_events"] = timed(launch_floor(mask.device), rounds, calls)
    rec["rays_py_events_again"] = timed(lambda: sampler(cams, mask=mask), rounds, calls)
    rec["torch_over_rays_py"] = round(rec["torch_events"]["median_ms"] / rec["rays_py_events"]["median_ms"], 3)
    rec["rays_py_over_launch_floor"] = round(rec["rays_py_events"]["median_ms"] / rec["launch_floor_events"]["median_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--mc-cameras", type=int, default=1280)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    lo, hi = 1.5, 5.5
    one, many = cameras(1, dev), cameras(a.mc_cameras, dev, seed=2)
    m1, mB = silhouettes(1, dev), silhouettes(a.mc_cameras, dev, seed=3)
    grid = rays.NDCMultinomialRaysampler(224, 224, 256, lo, hi)
    mc = rays.MonteCarloRaysampler(-1.0, 1.0, -1.0, 1.0, 30, 128, lo, hi, stratified_sampling=True, seed=1)
    rows = [case("masked 224x224 grid, one camera, 256 points (generateCors.py)", grid, one, m1,
                 lambda: torch_grid(one, m1, 256, lo, hi), a.rounds, a.calls),
            case(f"masked Monte-Carlo, {a.mc_cameras} cameras x 30 rays x 128 points, strata (genFeat.py)", mc, many, mB,
                 lambda: torch_mc(many, mB, 30, 128, lo, hi), a.rounds, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "rays.* masked bundles against the same steps in torch on the same device and against the launch floor "
                               "(three one-element fills and a 4-byte read); HIP events around `calls_per_round` calls, per call; one process",
                       "device": torch.cuda.get_device_name(0), "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
