"""The fine pass's depths (ops.resample_lengths, isr_resample_lengths) on the device, timed with HIP events:
    python tools/bench_resample.py [--out profiles/resample.json] [--rounds 7] [--calls 20]
  * 50 176 rays x 256 points, 256 samples, with the input samples (generateCors.py's 224 x 224 grid);
  * 38 400 rays x 128 points, 128 samples, with the input samples (genFeat.py's 1 280 cameras x 30 rays).
Each against
  * the same stage written in torch on the same device — the restatement of sample_pdf_python with torch.rand units, then
    the cat and the sort of pren.py:444-450 (torch's random stream, so other samples: the work is the same, the values are
    not compared);
  * the byte floor (2 N P + N P_out) * 4 bytes at the HBM rate one streaming copy reaches on this device, which this tool
    measures itself (a 256 MiB device-to-device copy: read + write) beside the 8 TB/s of the data sheet;
  * the launch floor: one one-element fill, what one launch costs whatever it computes.
Then the fine render of a (60, 256) radiance field on the 224 x 224 grid with 64 points — coarse render + resample + 128-point
render, renderer(..., stratified=True, add_input_samples=True) — against the coarse render alone.
A round is `calls` calls between two events, after one warm-up call of every route; the record holds the median, the
fastest and the slowest round per call.  The device result is compared with the host build before timing.  No threshold:
the record is the measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops, rays
from tests import resample_ref as rf
from tests.radiance_ref import device_field

HBM_SPEC = 8.0e12


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


def inputs(N, P, dev):
    """Gaussian-bump emission-absorption weights as in tests/resample_ref.parity_inputs, N rays."""
    reps = (N + 255) // 256
    ln, w = rf.parity_inputs(P)
    ln, w = np.tile(ln, (reps, 1))[:N], np.tile(w, (reps, 1))[:N]
    return ln, w, torch.from_numpy(ln).to(dev), torch.from_numpy(w).to(dev)


def torch_stage(lengths, weights, n):
    mids = 0.5 * (lengths[..., 1:] + lengths[..., :-1])
    u = torch.rand(lengths.shape[0], n, device=lengths.device)
    z = rf.sample_pdf_torch(mids, weights[..., 1:-1], u)
    return torch.sort(torch.cat((lengths, z), dim=-1), dim=-1)[0]


def copy_rate(dev, rounds, calls):
    a = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    t = timed(lambda: b.copy_(a), rounds, calls)
    return 2 * a.numel() / (t["median_ms"] * 1e-3), t


def case(name, N, P, n, dev, rate, rounds, calls):
    ln, w, ln_d, w_d = inputs(N, P, dev)
    got = ops.resample_lengths(ln_d, w_d, n, True, False, seed=1)
    check = slice(0, 2048)
    same = np.array_equal(got[check].cpu().numpy().view(np.uint32),
                          ops.resample_lengths_host(ln[check], w[check], n, True, False, seed=1).view(np.uint32))
    nbytes = (2 * N * P + N * (n + P)) * 4
    one = torch.empty(1, dtype=torch.int32, device=dev)
    rec = {"case": name, "rays": N, "P": P, "n": n, "P_out": n + P, "rays_per_workgroup": ops.resample_rays_per_group(P, n, True),
           "bytes": nbytes, "first_2048_rows_equal_host_build": bool(same)}
    rec["resample_events"] = timed(lambda: ops.resample_lengths(ln_d, w_d, n, True, False, seed=1), rounds, calls)
    rec["torch_events"] = timed(lambda: torch_stage(ln_d, w_d, n), rounds, calls)
    rec["launch_floor_events"] = timed(lambda: one.fill_(1), rounds, calls)
    rec["resample_events_again"] = timed(lambda: ops.resample_lengths(ln_d, w_d, n, True, False, seed=1), rounds, calls)
    rec["byte_floor_ms_at_measured_copy_rate"] = round(nbytes / rate * 1e3, 4)
    rec["byte_floor_ms_at_8_TB_s"] = round(nbytes / HBM_SPEC * 1e3, 4)
    ms = rec["resample_events"]["median_ms"]
    rec["torch_over_resample"] = round(rec["torch_events"]["median_ms"] / ms, 3)
    rec["resample_over_byte_floor_measured"] = round(ms / (nbytes / rate * 1e3), 3)
    rec["resample_over_launch_floor"] = round(ms / rec["launch_floor_events"]["median_ms"], 3)
    return rec


def render_case(dev, rounds, calls):
    P = 64
    field = device_field((60, 256, 2, 256, 3), dev, seed=5)
    cams = rays.PerspectiveCameras(torch.eye(3)[None], torch.tensor([[0.0, 0.0, 2.5]]), focal_length=2.0, in_ndc=True, device=dev)
    sampler = rays.NDCMultinomialRaysampler(224, 224, P, 1.0, 4.0)
    marcher = rays.EmissionAbsorptionRaymarcherStratified()
    coarse = rays.ImplicitRendererStratified(sampler, marcher, device=dev)
    fine = rays.ImplicitRendererStratified(sampler, marcher, device=dev, fine_seed=1)
    bundle = sampler(cams)
    rec = {"case": f"224 x 224 grid, {P} coarse points, (60, 256) radiance field with a 256-wide colour head",
           "rays": 224 * 224, "P": P, "P_fine": 2 * P}
    rec["coarse_render_events"] = timed(lambda: coarse(cams, field.batched_forward), rounds, calls)
    rec["fine_render_events"] = timed(lambda: fine(cams, field.batched_forward, stratified=True, add_input_samples=True), rounds, calls)
    w = field.render(bundle, threshold=-1.0, return_weights=True)[1]
    ln_d, w_d = bundle.lengths.reshape(-1, P).contiguous(), w.reshape(-1, P).contiguous()
    rec["resample_alone_events"] = timed(lambda: ops.resample_lengths(ln_d, w_d, P, True, False, seed=1), rounds, calls)
    rec["fine_over_coarse"] = round(rec["fine_render_events"]["median_ms"] / rec["coarse_render_events"]["median_ms"], 3)
    rec["resample_share_of_fine"] = round(rec["resample_alone_events"]["median_ms"] / rec["fine_render_events"]["median_ms"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    rate, copy_t = copy_rate(dev, a.rounds, 5)
    rows = [case("50 176 rays x 256 points, 256 samples, add_input (generateCors.py)", 50176, 256, 256, dev, rate, a.rounds, a.calls),
            case("38 400 rays x 128 points, 128 samples, add_input (genFeat.py)", 38400, 128, 128, dev, rate, a.rounds, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    render = render_case(dev, a.rounds, max(a.calls // 4, 2))
    print(json.dumps(render), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "ops.resample_lengths against the same stage in torch on the same device (torch's own random units: the "
                               "work is the same, the values are not compared), the byte floor (2 N P + N P_out) * 4 at this device's "
                               "measured copy rate and at the data sheet's 8 TB/s, and the launch floor (one one-element fill); then "
                               "the fine render against the coarse render.  HIP events around `calls_per_round` calls, per call; one "
                               "process",
                       "device": torch.cuda.get_device_name(0),
                       "copy_rate_bytes_per_s": round(rate), "copy_256MiB_events": copy_t,
                       "not_measured": "hardware counters (LDS bank conflicts, achieved occupancy, HBM bytes): the resident waves per "
                                       "SIMD in profiles/resample_resources.txt are arithmetic on the LDS size; the share of the kernel's "
                                       "time spent in the one-lane-per-ray scans and in the sort's barriers; shapes other than these; "
                                       "pytorch3d's own sample_pdf (not available)",
                       "cases": rows, "fine_render": render}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
