"""The optimiser's step + zero_grad at the two training programs' shapes, timed with HIP events:
    python tools/bench_adam.py [--out profiles/adam_step.json] [--rounds 7] [--calls 20]
  * the pose shape: the SIREN key field's tensors (3 -> 256 -> 256 -> 256 -> 12) in one group and, standing in for the
    ResNet-UNet that is not part of the package, a synthetic list of 150 tensors of about 20 M elements in all (convolution
    weights of growing width with their biases and norm vectors), generated here from a seed, in a second group with the
    ramp: trainPose.py:208-236;
  * the NeRF shape: two fields.TrainableRadianceField at the reference's widths, one group each: trainNerfFine.py:214.
Per shape, one iteration = step() then zero_grad(), gradients in place (filled once; Adam's time does not depend on values):
  optim.Adam with zero_in_step (zero_grad() launches nothing) and without (zero_grad(set_to_none=False): one launch);
  torch.optim.Adam with foreach=False, foreach=True and fused=True, each followed by zero_grad(set_to_none=False);
  the byte floor at the copy bandwidth measured here (a device-to-device copy of 256 MiB moves 2 bytes per byte copied):
  28 bytes per element (p, g, m, v read, p, m, v written), 32 with the gradient's zero;
  the launch floor: as many empty launches as the package makes (isr_fps_launch_floor), 2 with zero_in_step and 3 without.
A round is `calls` iterations between two events after a warm-up of every route; the record holds the median, the fastest
and the slowest round per iteration.  No threshold: the record is the measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, optim


def timed(fn, rounds, calls):
    for _ in range(3):
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


def synthetic_unet_shapes(seed=0, tensors=150, target=20_000_000):
    """150 shapes: 3 x 3 convolution weights whose widths grow 32 .. 512, each followed by a bias and two norm vectors, scaled so
    that the elements total about `target`."""
    rng = np.random.default_rng(seed)
    widths = np.linspace(32, 512, (tensors + 3) // 4).astype(int)
    shapes = []
    for cout in widths:
        cin = int(max(3, cout // int(rng.choice([1, 2]))))
        shapes += [(int(cout), cin, 3, 3), (int(cout),), (int(cout),), (int(cout),)]
    shapes = shapes[:tensors]
    total = sum(int(np.prod(s)) for s in shapes)
    scale = (target / total) ** 0.5
    out = []
    for s in shapes:
        out.append((max(1, int(s[0] * scale)), max(1, int(s[1] * scale)), 3, 3) if len(s) == 4 else (max(1, int(s[0] * scale)),))
    return out


def siren_shapes(hidden=256, layers=3, out=12):
    dims = [3] + [hidden] * layers + [out]
    return [s for a, b in zip(dims[:-1], dims[1:]) for s in ((b, a), (b,))]


def radiance_shapes():
    """trainNerfFine.py's field as fields.TrainableRadianceField holds it, taken from the class itself."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import fields
    from tests import density_ref as dr, radiance_ref as rr
    f = fields.TrainableRadianceField(*rr.fixture(60, 256, 2, 256, 3, seed=0), dr.frequencies(60), 10.0, torch.device("cuda:0"))
    return [tuple(p.shape) for p in f.parameters()]


def make_params(groups_of_shapes, dev, seed=0):
    gen = torch.Generator(device=dev).manual_seed(seed)
    groups = []
    for shapes in groups_of_shapes:
        ps = [torch.nn.Parameter(torch.randn(s, device=dev, generator=gen) * 0.1) for s in shapes]
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 0.01
        groups.append(ps)
    return groups


def copy_bandwidth(dev, rounds, calls):
    a = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    t = timed(lambda: b.copy_(a), rounds, calls)
    return 2 * a.numel() / (t["median_ms"] * 1e-3), t


def launch_floor(dev, launches, rounds, calls):
    L = _capi.lib()
    s = lambda: torch.cuda.current_stream(dev).cuda_stream
    return timed(lambda: _capi.check(L.isr_fps_launch_floor(launches, s()), "isr_fps_launch_floor"), rounds, calls)


def bench_shape(name, groups_of_shapes, group_kw, dev, bw, rounds, calls):
    n_tensors = sum(len(g) for g in groups_of_shapes)
    elements = sum(int(np.prod(s)) for g in groups_of_shapes for s in g)
    rec = {"tensors": n_tensors, "elements": elements, "groups": len(groups_of_shapes)}

    def ours(zero_in_step):
        ps = make_params(groups_of_shapes, dev)
        opt = optim.Adam([{"params": p, **kw} for p, kw in zip(ps, group_kw)], zero_in_step=zero_in_step)

        def it():
            opt.step()
            opt.zero_grad() if zero_in_step else opt.zero_grad(set_to_none=False)
        return it

    def torchs(**flags):
        ps = make_params(groups_of_shapes, dev)
        opt = torch.optim.Adam([{"params": p, "lr": kw["lr"]} for p, kw in zip(ps, group_kw)], **flags)

        def it():
            opt.step()
            opt.zero_grad(set_to_none=False)
        return it

    rec["optim_adam_zero_in_step"] = timed(ours(True), rounds, calls)
    rec["optim_adam"] = timed(ours(False), rounds, calls)
    rec["torch_adam_single_tensor"] = timed(torchs(foreach=False), rounds, max(2, calls // 4))
    rec["torch_adam_foreach"] = timed(torchs(foreach=True), rounds, calls)
    rec["torch_adam_fused"] = timed(torchs(fused=True), rounds, calls)
    rec["byte_floor_ms"] = {"28_bytes_per_element": round(28 * elements / bw * 1e3, 4), "32_bytes_per_element": round(32 * elements / bw * 1e3, 4)}
    rec["launch_floor"] = {"2_launches": launch_floor(dev, 2, rounds, calls), "3_launches": launch_floor(dev, 3, rounds, calls)}
    print(name, json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_step.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_adam.py measures on the GPU; there is no fallback"
    dev = torch.device("cuda:0")
    bw, bw_t = copy_bandwidth(dev, a.rounds, a.calls)
    rec = {"device": torch.cuda.get_device_name(0), "copy_bandwidth_bytes_per_s": bw, "copy_256MiB": bw_t,
           "iteration": "step() then zero_grad(); gradients stay in place"}
    pose_kw = [dict(lr=optim.LR_MLP, ramp_steps=optim.RAMP_STEPS), dict(lr=optim.LR_CNN, ramp_steps=optim.RAMP_STEPS)]
    rec["pose"] = bench_shape("pose", [siren_shapes(), synthetic_unet_shapes()], pose_kw, dev, bw, a.rounds, a.calls)
    rs = radiance_shapes()
    nerf_kw = [dict(lr=optim.LR_NERF), dict(lr=optim.LR_NERF)]
    rec["nerf"] = bench_shape("nerf", [rs, rs], nerf_kw, dev, bw, a.rounds, a.calls)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
