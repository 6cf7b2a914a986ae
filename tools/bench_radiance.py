"""The radiance field's fused render (fields.RadianceField.render, isr_radiance_render) against the reference's route:
    python tools/bench_radiance.py [--out profiles/radiance_render.json] [--reps 5] [--rays 50176] [--points 256]
H = 60, 360 -> 256 -> 256 -> 1 with the colour head 616 -> 256 -> 3, Softplus(10); 50 176 rays x 256 points: one
generateCors.py image (224 x 224 rays).  tools/bench_density.py's method, HIP events, median and spread over `reps` after one
warm-up call, every route in the same process on the same inputs:
  * the fused soft render (threshold < 0: every point evaluated);
  * the threshold render (0.2: the tiles behind a ray's first hit are skipped);
  * isr_density_march alone in both modes, which gives the colour head's cost on top;
  * the same layers as a torch module on the device, the points made by torch and pushed through in 16 chunks
    (batched_forward, nerf.py:458-521), then the raymarcher's statements (pren.py:338-369) in torch;
  * the algorithmic multiply-adds, 2 P N (6H 256 + 256 256 + 256 Wc + Wc C) + 2 N 6H Wc, over the f32 matrix peak.
No threshold: the record is the measurement."""
import argparse, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
from bench_render import event_timed, stats
from tests.density_ref import frequencies, torch_march
from tests.radiance_ref import TorchRadiance, device_field, fixture

PEAK_F32_MATRIX = 157.3e12          # MI355X, v_mfma_f32_32x32x2_f32
NET = (60, 256, 2, 256, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=224 * 224)
    ap.add_argument("--points", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    H, hidden, _, Wc, C = NET
    field = device_field(NET, dev, seed=5)
    module = TorchRadiance(fixture(*NET, seed=5), frequencies(H)).to(dev)
    rng = np.random.default_rng(5)
    N, P = a.rays, a.points
    o = rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32)
    d = (rng.normal(size=(N, 3)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    ln = np.sort(rng.uniform(0.0, 1.5, (N, P)).astype(np.float32), axis=1)
    to, td, tl = (torch.from_numpy(x).to(dev) for x in (o, d, ln))
    ws = torch.empty((ops.radiance_workspace_bytes(N, Wc),), dtype=torch.uint8, device=dev)
    render = lambda thr: ops.radiance_render(field.rpack, field.widths, H, Wc, C, to, td, tl, threshold=thr, workspace=ws)
    march = lambda thr, dens: ops.density_march(field.pack, field.widths, H, to, td, tl, thr, want_densities=dens)

    def reference_route(thr=-1.0):
        dens, col = [], []
        for co, cd, cl in zip(torch.chunk(to, 16), torch.chunk(td, 16), torch.chunk(tl, 16)):
            rho, c = module(co, cd, cl)
            dens.append(rho[..., 0])
            col.append(c)
        rho, col = torch.cat(dens), torch.cat(col)
        w, _ = torch_march(rho, tl, thr)
        c = (rho > thr).float() if thr >= 0 else rho
        return torch.cat(((w[..., None] * col).sum(dim=-2), 1.0 - torch.prod(1.0 - c, dim=-1, keepdim=True)), dim=-1), rho

    got = render(-1.0)["image"]
    ref, rho = reference_route()
    torch.cuda.synchronize()
    # the opacity depends on the densities alone; the features also on the direction's embedding, where at H = 60 the last
    # bit of a normalised direction is many periods of the top frequencies: torch's normalize on the device need not be the
    # CPU's bits, so its colours are another function's values and their difference bounds nothing
    diff_opacity = float((got[:, -1] - ref[:, -1]).abs().max())
    diff_features = float((got[:, :-1] - ref[:, :-1]).abs().max())
    for warm in (lambda: render(0.2), lambda: march(0.2, True), lambda: march(0.2, False)):
        warm()
    t_soft = stats(event_timed(lambda: render(-1.0), a.reps))
    t_thr = stats(event_timed(lambda: render(0.2), a.reps))
    t_march_full = stats(event_timed(lambda: march(0.2, True), a.reps))
    t_march_thr = stats(event_timed(lambda: march(0.2, False), a.reps))
    t_ref = stats(event_timed(reference_route, a.reps))
    flop = 2.0 * P * N * (6 * H * hidden + hidden * hidden + hidden * Wc + Wc * C) + 2.0 * N * 6 * H * Wc
    row = {"rays": N, "points_per_ray": P, "H": H, "hidden": [hidden, hidden], "Wc": Wc, "C": C, "flop_every_point": flop,
           "share_of_points_above_threshold": round(float((rho > 0.2).float().mean()), 4),
           "isr_radiance_render_soft_events": t_soft, "isr_radiance_render_threshold_events": t_thr,
           "isr_density_march_every_point_events": t_march_full, "isr_density_march_threshold_events": t_march_thr,
           "torch_16_chunks_and_torch_march_events": t_ref,
           "soft_tflops": round(flop / (t_soft["median_ms"] * 1e-3) / 1e12, 2),
           "soft_share_of_f32_matrix_peak": round(flop / (t_soft["median_ms"] * 1e-3) / PEAK_F32_MATRIX, 4),
           "soft_render_over_density_march_every_point": round(t_soft["median_ms"] / t_march_full["median_ms"], 3),
           "threshold_render_over_density_march_threshold": round(t_thr["median_ms"] / t_march_thr["median_ms"], 3),
           "torch_over_soft_render": round(t_ref["median_ms"] / t_soft["median_ms"], 3),
           "torch_over_threshold_render": round(t_ref["median_ms"] / t_thr["median_ms"], 3),
           "largest_opacity_difference_from_torch": diff_opacity,
           "largest_feature_difference_from_torch_device_normalize": diff_features}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "isr_radiance_render against isr_density_march and against the same layers as a torch module in 16 "
                               "chunks with the torch march, one process, same inputs", "device": torch.cuda.get_device_name(0),
                       "f32_matrix_peak_flops": PEAK_F32_MATRIX, "render": row}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
