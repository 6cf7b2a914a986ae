"""The ray losses (losses.distortion_loss and losses.render_loss: include/isr_ray_losses.h), forward plus backward, timed with
HIP events:
    python tools/bench_ray_losses.py [--out profiles/ray_losses.json] [--rounds 7] [--calls 20]
  * distortion loss at (N, P) = (1 200, 64) and (1 200, 128), trainNerfFine.py's 3 x 400 rays at its coarse and fine sample
    counts, and (50 176, 256), its 224 x 224 grid render;
  * render loss at trainNerfFine.py's shape: B = 3 images, n = 400 rays each, F = 3, 224 x 224 targets.
Each against
  * the reference's expressions under torch autograd on the same device and the same inputs (tests/ray_losses_ref.py's
    torch_formula, which stores every pair, and torch_render_terms: grid_sample and the elementwise chain).  Where torch cannot
    hold the pair tensors of a shape, it is timed on the largest power-of-two ray count that runs, and that count is recorded;
  * the launch floor: as many one-element fills as the fused route launches kernels;
  * the byte floor: the bytes the rule has to move (the inputs once per pass and the gradient once) over 8 TB/s.
Peak memory (torch.cuda.max_memory_allocated beyond what was allocated before the call) of both routes and whether two fused
calls give identical bytes go into the same record.  A round is `calls` forward+backward calls between two events, after one
warm-up call of every route; the record holds the median, the fastest and the slowest round per call.  No threshold: the
record is the measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import losses
from tests import ray_losses_ref as ref

HBM_BYTES_PER_S = 8.0e12


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


def peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def launch_floor(count, dev, rounds, calls):
    one = torch.empty(1, dtype=torch.int32, device=dev)
    return timed(lambda: [one.fill_(1) for _ in range(count)], rounds, calls)


def finish(rec, fused_launches, floor_bytes, dev, rounds, calls):
    ms = rec["fused_events"]["median_ms"]
    rec["launch_floor_events"] = {"fills": fused_launches, **launch_floor(fused_launches, dev, rounds, calls)}
    rec["byte_floor_ms"] = round(floor_bytes / HBM_BYTES_PER_S * 1e3, 6)
    rec["byte_floor_assumes"] = f"{floor_bytes} bytes at 8 TB/s"
    rec["fused_over_launch_floor"] = round(ms / rec["launch_floor_events"]["median_ms"], 2)
    rec["fused_over_byte_floor"] = round(ms / rec["byte_floor_ms"], 1)
    t = rec["torch_events"]["median_ms"]
    part = rec.get("torch_rays", rec.get("N")) != rec.get("N")      # torch ran on a part of the rays: scale its time to all
    if part:
        t *= rec["N"] / rec["torch_rays"]
    rec["torch_over_fused_scaled_to_all_rays" if part else "torch_over_fused"] = round(t / ms, 2)
    if t < ms:
        rec["verdict"] = "THE FUSED ROUTE IS SLOWER THAN TORCH HERE"
    return rec


def distortion_case(name, N, P, dev, rounds, calls):
    rng = np.random.default_rng(1)
    lengths = torch.from_numpy(ref.fine_depths(rng, N, P)).to(dev)
    weights = torch.from_numpy(ref.march_weights(rng, N, P, 64.0 / P)).to(dev).requires_grad_(True)

    def fused():
        weights.grad = None
        losses.distortion_loss(lengths, weights).backward()

    rec = {"case": name, "N": N, "P": P, "pairs": N * (P - 1) ** 2, "pair_tensor_bytes_each": 4 * N * (P - 1) ** 2}
    fused()
    ours = weights.grad.clone()
    fused()
    rec["two_calls_identical_bytes"] = bool(torch.equal(ours.view(torch.int32), weights.grad.view(torch.int32)))
    rec["fused_events"] = timed(fused, rounds, calls)
    rec["fused_peak_bytes"] = peak(fused, dev)
    n = N
    while True:                                               # the largest ray count whose pair tensors torch can hold
        lt, wt = lengths[:n], weights.detach()[:n].clone().requires_grad_(True)

        def reference():
            wt.grad = None
            ref.torch_formula(lt, wt).backward()

        try:
            reference()
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            del wt
            torch.cuda.empty_cache()
            n //= 2
    rec["torch_rays"] = n
    scale = n / N                                             # torch's mean is over n rays: its gradient is N / n times ours
    rec["largest_gradient_difference_from_torch_relative_to_the_largest_gradient"] = float(
        (ours[:n] - wt.grad * scale).abs().max() / (wt.grad * scale).abs().max())
    rec["torch_events"] = timed(reference, rounds, max(calls // 4, 2))
    rec["torch_peak_bytes"] = peak(reference, dev)
    rec["fused_events_again"] = timed(fused, rounds, calls)
    launches = 1 + (1 if N <= 256 else 2) + 1                 # rays, the levels of the mean, backward
    return finish(rec, launches, 5 * 4 * N * P + 8 * N, dev, rounds, calls)


def render_case(name, B, n, F, H, W, dev, rounds, calls):
    rng = np.random.default_rng(2)
    rendered, images, sils, xys = (torch.from_numpy(a).to(dev) for a in ref.render_case(rng, B, n, F, H, W, special=False))
    xys = (xys / 1.2).contiguous()                            # the sampler's rays: all inside
    rendered.requires_grad_(True)

    def fused():
        rendered.grad = None
        c, s = losses.render_loss(rendered, images, sils, xys)
        (c + s).backward()

    def reference():
        rendered.grad = None
        c, s = ref.torch_render_terms(rendered, images, sils, xys)
        (c + s).backward()

    rec = {"case": name, "B": B, "n": n, "F": F, "H": H, "W": W}
    fused()
    ours = rendered.grad.clone()
    fused()
    rec["two_calls_identical_bytes"] = bool(torch.equal(ours.view(torch.int32), rendered.grad.view(torch.int32)))
    reference()
    rec["largest_gradient_difference_from_torch_relative_to_the_largest_gradient"] = float(
        (ours - rendered.grad).abs().max() / rendered.grad.abs().max())
    x64 = rendered.detach().double().requires_grad_(True)    # torch-f32's h rounds to 0 below |d| = 3.5e-5 and abs() stops the gradient
    c, s = ref.torch_render_terms(x64, images.double(), sils.double(), xys.double())
    (c + s).backward()
    rec["the_same_against_torch_in_f64"] = float((ours.double() - x64.grad).abs().max() / x64.grad.abs().max())
    rec["fused_events"] = timed(fused, rounds, calls)
    rec["torch_events"] = timed(reference, rounds, calls)
    rec["fused_events_again"] = timed(fused, rounds, calls)
    rec["fused_peak_bytes"] = peak(fused, dev)
    rec["torch_peak_bytes"] = peak(reference, dev)
    rec["fused_kernels"] = 1 + (0 if B * n <= 256 else 1) + 1
    rec["fused_route_also_launches"] = "torch's two selects of out, their sum and the backward of those: the (c + s) of this benchmark"
    rows = B * n
    return finish(rec, rec["fused_kernels"], rows * (4 * (F + 1) * 3 + 2 * 8 + 2 * 4 * (F + 1)), dev, rounds, calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    busy = torch.rand(4096, 4096, device=dev)
    for _ in range(200):                                      # about a second of work first: clocks and code objects
        busy = (busy @ busy).clamp_(0, 1)
    torch.cuda.synchronize()
    rows = [distortion_case("trainNerfFine.py's coarse pass: 3 x 400 rays, 64 samples", 1200, 64, dev, a.rounds, a.calls),
            distortion_case("trainNerfFine.py's fine pass at 128 samples: 3 x 400 rays", 1200, 128, dev, a.rounds, a.calls),
            distortion_case("the grid render: 224 x 224 rays, 256 samples", 50176, 256, dev, a.rounds, a.calls),
            distortion_case("the coarse pass once more, after everything else", 1200, 64, dev, a.rounds, a.calls),
            render_case("trainNerfFine.py's Huber terms of one render: 3 x 400 rays, 224 x 224 targets", 3, 400, 3, 224, 224, dev,
                        a.rounds, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "losses.distortion_loss(lengths, weights).backward() and losses.render_loss(...) + backward against the "
                               "reference's expressions under torch autograd on the same device and inputs, the launch floor (as many "
                               "one-element fills as the fused route launches kernels) and the byte floor (the rule's bytes at 8 TB/s).  "
                               "HIP events around `calls_per_round` forward+backward calls, per call; one process; peak bytes beyond "
                               "what was allocated before the call",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "the kernels apart; hardware counters (VALU and LDS utilisation, occupancy); P other than 64, "
                                       "128, 256; the losses inside training.nerf_train_step at the reference's shape; f64 issue rate "
                                       "as a floor of the pair loop",
                       "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
