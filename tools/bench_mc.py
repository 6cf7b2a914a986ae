"""Iso-surface extraction on the device (ops.marching_cubes: isr_mc_count + isr_mc_emit) at the reference's grid:
    python tools/bench_mc.py [--out profiles/mc_extract.json] [--reps 20] [--res 128] [--threshold 0.05]
res = 128 on the synthetic DensityField of tools/bench_density.py (H = 60, 360 -> 256 -> 256 -> 1, Softplus(10)); a smooth
ball-plus-ripple volume of the same size beside it, since random weights give a far busier surface than a trained field.
  * isr_mc_count, isr_mc_emit and the two back to back, on outputs sized beforehand — HIP events around the C calls, the
    median and the min-max spread over `reps` after a warm-up call; the one read of the totals between the two phases is the
    caller's synchronise and is timed apart, as the whole of ops.marching_cubes on a host clock.  A round is 50 calls
    between one pair of events, divided by 50;
  * grid_densities(res) in the same run, HIP events;
  * the bytes the two phases must move — the volume once per phase (4 N each), the slot words written and read (2 N each),
    the workgroups' offsets, the outputs (24 V + 12 F) — over the HBM rate a copy reaches on this chip: the floor;
  * the launch floor: the same number of launches (3) of an empty kernel, HIP events.
There is no earlier figure and no mcubes here to compare with: the record is the measurement, nothing is gated."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
from bench_render import event_timed, stats
from tests.density_ref import fixture, frequencies
from tests.mc_ref import ripple_ball

HBM_COPY_RATE = 6.29e12             # bytes / s, MI355X: what a float4 copy reaches (8.0e12 is the data-sheet figure)
LAUNCHES = 3                        # count, scan, emit
BLOCK = 256                         # points per workgroup (csrc/mc_extract.hip)


INNER = 50                          # calls between one pair of events: a window of milliseconds, not of one short call


def per_call(fn, reps):
    def many():
        for _ in range(INNER):
            fn()
    st = stats([ms / INNER for ms in event_timed(many, reps)])
    st["calls_per_round"] = INNER
    return st


def phases(vol, iso, reps):
    """-> (V, F, timings of count, emit and both) for a device volume."""
    L = _capi.lib()
    dev = vol.device
    nx, ny, nz = vol.shape
    ws = torch.empty(L.isr_mc_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    st = lambda: torch.cuda.current_stream(dev).cuda_stream

    def count():
        _capi.check(L.isr_mc_count(vol.data_ptr(), nx, ny, nz, iso, counts.data_ptr(), ws.data_ptr(), ws.numel(), st()), "isr_mc_count")
    count()
    V, F = (int(c) for c in counts.cpu())
    verts = torch.empty((max(V, 1), 3), dtype=torch.float64, device=dev)
    tris = torch.empty((max(F, 1), 3), dtype=torch.int32, device=dev)

    def emit():
        _capi.check(L.isr_mc_emit(vol.data_ptr(), nx, ny, nz, iso, ws.data_ptr(), ws.numel(), verts.data_ptr(), V, tris.data_ptr(), F,
                                  st()), "isr_mc_emit")

    def both():
        count()
        emit()
    both()
    torch.cuda.synchronize()
    return V, F, {"isr_mc_count_events": per_call(count, reps), "isr_mc_emit_events": per_call(emit, reps),
                  "count_then_emit_events": per_call(both, reps)}


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def row(name, vol, iso, reps):
    N = vol.numel()
    V, F, t = phases(vol, iso, reps)
    nb = -(-N // BLOCK)
    must = 2 * 4 * N + 2 * 2 * N + 3 * 8 * nb + 24 * V + 12 * F
    floor_ms = must / HBM_COPY_RATE * 1e3
    ops.marching_cubes(vol, iso)
    t["ops_marching_cubes_wall_with_its_read_of_the_totals"] = wall(lambda: ops.marching_cubes(vol, iso, check_finite=False), reps)
    both = t["count_then_emit_events"]["median_ms"]
    return dict({"volume": name, "shape": list(vol.shape), "iso": iso, "vertices": V, "triangles": F, "bytes_that_must_move": must,
                 "hbm_floor_ms": round(floor_ms, 5), "count_then_emit_over_hbm_floor": round(both / floor_ms, 2)}, **t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--threshold", type=float, default=0.05)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    H, hidden = 60, 256
    Ws, bs = fixture(H, hidden, 2, seed=5)
    field = DensityField(Ws, bs, frequencies(H), 10.0, dev)
    grid = field.grid_densities(a.res)
    torch.cuda.synchronize()
    t_grid = stats(event_timed(lambda: field.grid_densities(a.res), max(a.reps // 4, 3)))
    L = _capi.lib()
    floor = lambda: _capi.check(L.isr_fps_launch_floor(LAUNCHES, torch.cuda.current_stream(dev).cuda_stream), "isr_fps_launch_floor")
    floor()
    torch.cuda.synchronize()
    t_floor = per_call(floor, a.reps)
    rows = [row("synthetic DensityField (random weights)", grid, a.threshold, a.reps),
            row("ball plus ripple", torch.from_numpy(ripple_ball(a.res)).to(dev), 0.0, a.reps)]
    for r in rows:
        r["count_then_emit_over_launch_floor"] = round(r["count_then_emit_events"]["median_ms"] / t_floor["median_ms"], 2)
        r["count_then_emit_over_grid_densities"] = round(r["count_then_emit_events"]["median_ms"] / t_grid["median_ms"], 5)
    rec = {"what": "isr_mc_count + isr_mc_emit at the reference's grid size, HIP events after warm-up; the floors beside them",
           "device": torch.cuda.get_device_name(0), "res": a.res, "hbm_copy_rate_bytes_per_s": HBM_COPY_RATE,
           "grid_densities_events": t_grid, f"launch_floor_{LAUNCHES}_empty_kernels_events": t_floor, "volumes": rows}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
