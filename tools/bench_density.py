"""The density field's ray march (fields.DensityField.surface_points, isr_density_march) against the reference's route:
    python tools/bench_density.py [--out profiles/density_march.json] [--reps 5] [--rays 50176] [--points 256]
H = 60, 360 -> 256 -> 256 -> 1, Softplus(10); 50 176 rays x 256 points: one generateCors.py image (224 x 224 rays).
  * one surface_points call (threshold 0.2: the tiles after a ray's first hit are skipped) and one with the densities asked
    for (every point evaluated) — HIP events, median and spread over `reps` after one warm-up call;
  * the same layers as a torch module on the device, the points made by torch and pushed through in 16 chunks
    (batched_forward_fordensity, nerf.py), then the cumprod march of pren.py:342-365 and the callers' max — HIP events;
  * the full evaluation's multiply-adds (360 * 256 + 256 * 256 + 256 per point, x 2) over the f32 matrix peak.
Both routes run in the same process on the same inputs; the largest difference between their points is recorded.
No threshold: the record is the measurement."""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
from bench_render import event_timed, stats
from tests.density_ref import TorchDensity, fixture, frequencies, torch_march

PEAK_F32_MATRIX = 157.3e12          # MI355X, v_mfma_f32_32x32x2_f32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=224 * 224)
    ap.add_argument("--points", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    H, hidden = 60, 256
    Ws, bs = fixture(H, hidden, 2, seed=5)
    field = DensityField(Ws, bs, frequencies(H), 10.0, dev)
    module = TorchDensity(Ws, bs, frequencies(H)).to(dev)
    rng = np.random.default_rng(5)
    N, P = a.rays, a.points
    o = rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32)
    d = rng.normal(size=(N, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = np.sort(rng.uniform(0.0, 1.5, (N, P)).astype(np.float32), axis=1)
    to, td, tl = (torch.from_numpy(x).to(dev) for x in (o, d, ln))

    def ours():
        return field.surface_points(to, td, tl, threshold=0.2)

    def ours_full():
        return ops.density_march(field.pack, field.widths, field.H, to, td, tl, 0.2, want_densities=True)

    def reference_route():
        pts = (to[:, None, :] + td[:, None, :] * tl[:, :, None]).reshape(-1, 3)
        rho = torch.cat([module(c)[..., 0] for c in torch.chunk(pts, 16)]).view(N, P)
        w, depth = torch_march(rho, tl, 0.2)
        return to + td * depth[:, None], rho

    got = ours()[0]
    ref, rho = reference_route()
    torch.cuda.synchronize()
    near = ((rho - 0.2).abs() <= 1e-6).any(dim=1)
    differ = int(((got != ref).any(dim=1) & ~near).sum())
    t_skip = stats(event_timed(ours, a.reps))
    t_full = stats(event_timed(ours_full, a.reps))
    t_ref = stats(event_timed(reference_route, a.reps))
    flop = float(N) * P * ops.density_flops(field.widths, H)
    row = {"rays": N, "points_per_ray": P, "H": H, "hidden": [hidden, hidden], "flop_every_point": flop,
           "share_of_points_above_threshold": round(float((rho > 0.2).float().mean()), 4),
           "isr_density_march_threshold_events": t_skip, "isr_density_march_every_point_events": t_full,
           "torch_16_chunks_and_cumprod_march_events": t_ref,
           "every_point_tflops": round(flop / (t_full["median_ms"] * 1e-3) / 1e12, 2),
           "every_point_share_of_f32_matrix_peak": round(flop / (t_full["median_ms"] * 1e-3) / PEAK_F32_MATRIX, 4),
           "torch_over_march_every_point": round(t_ref["median_ms"] / t_full["median_ms"], 3),
           "torch_over_march_threshold": round(t_ref["median_ms"] / t_skip["median_ms"], 3),
           "rays_whose_point_differs_from_torch": differ, "rays_within_1e-6_of_the_threshold": int(near.sum())}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "isr_density_march against the same layers as a torch module in 16 chunks and the torch march, one "
                               "process, same inputs", "device": torch.cuda.get_device_name(0),
                       "f32_matrix_peak_flops": PEAK_F32_MATRIX, "march": row}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
