"""The sequence ingest on the device (ops.ingest_views), timed with HIP events:
    python tools/bench_ingest.py [--out profiles/ingest.json] [--rounds 7] [--calls 3]
Shapes: 1 280 frames of 640 x 480 at maxB 200 and 224 (ruapc's sequence), 500 frames of 720 x 540 at 224 (T-LESS's); disc masks
of three equal channels holding 0/255, random colours, all made on the device.  Against
  (a) the same steps composed from torch ops on the device, 64 frames at a time: the gate by multiplication, the box from amax /
      argmax over rows and columns, an affine grid from the box and grid_sample (bilinear, zeros outside) of the four planes,
      the camera in f64 — no host read, as the package; its bytes differ (f32 sampling, no even cut, a zero border): the same
      work, not the same bytes;
  (b) host loops of the rule over the first `--host-frames` frames, per frame: tests/ingest_ref.py's NumPy restatement, and
      NumPy with PIL's BILINEAR resize in place of the restatement's (PIL's bytes differ: it widens its support when shrinking);
  (c) the byte floor: the mask once for the box pass (n H W Cm), the boxes' footprint of rgb and mask once, the outputs once,
      at the bandwidth of a device-to-device copy of 1 GiB measured in the same run (read + write counted);
  (d) the floor of its empty launches (isr_ingest_launch_floor: the same three grids, empty kernels).
A round is `calls` calls between two events after one warm-up call; the record holds the median, the fastest and the slowest
round per call, whether two calls give identical bytes, and the peak memory above inputs and outputs.  No threshold: the record
is the measurement."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
from tests import ingest_ref as ir

SHAPES = ((1280, 480, 640, 200), (1280, 480, 640, 224), (500, 540, 720, 224))      # n, H, W, maxB
OFFSET, CM, TORCH_CHUNK = 5, 3, 64


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


def inputs(dev, n, H, W):
    g = torch.Generator(device=dev).manual_seed(n + H)
    rgb = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    cx = torch.randint(W // 4, 3 * W // 4, (n, 1, 1), device=dev, generator=g)
    cy = torch.randint(H // 4, 3 * H // 4, (n, 1, 1), device=dev, generator=g)
    rad = torch.randint(H // 12, H // 4, (n, 1, 1), device=dev, generator=g)
    yy, xx = torch.arange(H, device=dev)[None, :, None], torch.arange(W, device=dev)[None, None, :]
    disc = ((xx - cx) ** 2 + (yy - cy) ** 2 <= rad ** 2)
    mask = (disc.to(torch.uint8) * 255)[..., None].expand(n, H, W, CM).contiguous()
    K = torch.tensor([572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0], dtype=torch.float64, device=dev).repeat(n, 1)
    return rgb, mask, K.reshape(n, 3, 3)


def torch_route(rgb, mask, K, maxB):
    n, H, W, _ = rgb.shape
    dev = rgb.device
    d = (torch.arange(maxB, device=dev, dtype=torch.float32) + 0.5) / maxB      # the canvas coordinate over side, at pixel centres

    def run():
        outs = []
        for c0 in range(0, n, TORCH_CHUNK):
            r, m, k = rgb[c0:c0 + TORCH_CHUNK], mask[c0:c0 + TORCH_CHUNK], K[c0:c0 + TORCH_CHUNK].clone()
            nz = m[..., 0] != 0
            cols, rows = nz.any(1), nz.any(2)
            x2, y2 = cols.to(torch.uint8).argmax(1), rows.to(torch.uint8).argmax(1)
            w2 = W - cols.flip(1).to(torch.uint8).argmax(1) - x2
            h2 = H - rows.flip(1).to(torch.uint8).argmax(1) - y2
            w2, h2 = w2 - w2 % 2, h2 - h2 % 2
            hw, hh = w2 // 2, h2 // 2
            side = torch.maximum(w2, h2) + 2 * OFFSET
            hs1 = side // 2
            planes = torch.cat([r * (m != 0), m[..., :1]], 3).permute(0, 3, 1, 2).to(torch.float32)
            sx = d[None, :] * side[:, None] - (hs1 - hw)[:, None] + x2[:, None]      # source pixel-centre coordinates
            sy = d[None, :] * side[:, None] - (hs1 - hh)[:, None] + y2[:, None]
            grid = torch.stack([(sx / W * 2 - 1)[:, None, :].expand(-1, maxB, -1), (sy / H * 2 - 1)[:, :, None].expand(-1, -1, maxB)], 3)
            out = torch.nn.functional.grid_sample(planes, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            out = (out.round() / 255).permute(0, 2, 3, 1)
            k[:, 0, 2] += (-x2 + hs1 - hw)
            k[:, 1, 2] += (-y2 + hs1 - hh)
            k = k * maxB / side[:, None, None]
            k[:, 2, 2] = 1
            K4 = torch.zeros((k.shape[0], 4, 4), dtype=torch.float64, device=dev)
            K4[:, :3, :3] = k
            K4[:, 3, 2] = K4[:, 2, 3] = 1
            outs.append((out[..., :3].contiguous(), out[..., 3].contiguous(), K4))
        return [torch.cat(x) for x in zip(*outs)]

    return run


def host_loops(rgb, mask, K, maxB, frames):
    from PIL import Image
    r, m, k = rgb[:frames].cpu().numpy(), mask[:frames].cpu().numpy(), K[:frames].cpu().numpy().reshape(frames, 9)
    t0 = time.perf_counter()
    ir.ingest(r, m, k, maxB, OFFSET, False, "linear")
    t1 = time.perf_counter()
    for i in range(frames):
        g = ir.geometry(ir.bounding_rect(m[i, :, :, 0]), OFFSET)
        sq, sm = ir.canvases(r[i], m[i], g)
        np.asarray(Image.fromarray(sq).resize((maxB, maxB), Image.BILINEAR), np.float32) / np.float32(255)
        np.asarray(Image.fromarray(sm).resize((maxB, maxB), Image.BILINEAR), np.float32) / np.float32(255)
        ir.camera(k[i], g, maxB, False)
    t2 = time.perf_counter()
    return {"frames": frames, "numpy_restatement_ms_per_frame": round((t1 - t0) * 1e3 / frames, 3),
            "numpy_pil_ms_per_frame": round((t2 - t1) * 1e3 / frames, 3)}


def copy_bandwidth(dev, rounds):
    a = torch.empty(1 << 30, dtype=torch.uint8, device=dev).fill_(1)
    b = torch.empty_like(a)
    t = timed(lambda: b.copy_(a), rounds, 4)
    return 2 * (1 << 30) / (t["median_ms"] * 1e-3), t


def peak_above(fn, out_bytes):
    torch.cuda.synchronize()
    ops.clear_workspaces()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    del r
    return int(torch.cuda.max_memory_allocated() - base - out_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=24)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    bw, bw_t = copy_bandwidth(dev, a.rounds)
    rec = {"copy_bandwidth_bytes_per_s": round(bw, -9), "copy_1GiB_events": bw_t, "geometry": ops.ingest_geometry(), "shapes": []}
    print(json.dumps({"copy_bandwidth_TB_per_s": round(bw / 1e12, 3)}), flush=True)
    for n, H, W, maxB in SHAPES:
        rgb, mask, K = inputs(dev, n, H, W)
        pk = lambda: ops.ingest_views(rgb, mask, K, maxB, OFFSET, False, "linear")
        tc = torch_route(rgb, mask, K, maxB)
        v = pk()
        geom = v.geom.cpu().numpy().astype(np.int64)
        assert int(v.status.sum()) == 0
        out_bytes = n * maxB * maxB * 16 + n * (128 + 32 + 4)
        footprint = int((geom[:, 2] * geom[:, 3]).sum()) * (3 + CM)
        nbytes = n * H * W * CM + footprint + out_bytes + n * 72
        r = {"n": n, "H": H, "W": W, "Cm": CM, "maxB": maxB, "offset": OFFSET, "strips": ops.ingest_strips(H, W, CM)[1],
             "median_side": int(np.median(geom[:, 6])), "workspace_bytes": ops.ingest_workspace_bytes(n, H, W, CM)}
        r["package_events"] = timed(pk, a.rounds, a.calls)
        r["torch_events"] = timed(tc, a.rounds, 1)
        r["launch_floor_events"] = timed(lambda: ops.ingest_launch_floor(n, H, W, CM, maxB, dev), a.rounds, a.calls)
        r["package_events_again"] = timed(pk, a.rounds, a.calls)
        r["nearest_silhouette_events"] = timed(lambda: ops.ingest_views(rgb, mask, K, maxB, OFFSET, False, "nearest"), a.rounds, a.calls)
        r["host_loops"] = host_loops(rgb, mask, K, maxB, a.host_frames)
        ms = r["package_events"]["median_ms"]
        r["byte_floor_bytes"] = {"box_pass_mask": n * H * W * CM, "box_footprint_rgb_and_mask": footprint, "outputs": out_bytes}
        r["byte_floor_ms"] = round(nbytes / bw * 1e3, 4)
        r["package_over_byte_floor"] = round(ms / r["byte_floor_ms"], 2)
        r["package_over_launch_floor"] = round(ms / r["launch_floor_events"]["median_ms"], 2)
        r["torch_over_package"] = round(r["torch_events"]["median_ms"] / ms, 2)
        r["host_numpy_restatement_over_package"] = round(r["host_loops"]["numpy_restatement_ms_per_frame"] * n / ms, 1)
        r["host_numpy_pil_over_package"] = round(r["host_loops"]["numpy_pil_ms_per_frame"] * n / ms, 1)
        r["package_us_per_frame"] = round(ms * 1e3 / n, 3)
        x, y = pk(), pk()
        r["package_two_calls_identical_bytes"] = all(torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8)) for p, q in zip(x, y))
        del x, y, v
        r["package_peak_bytes_above_inputs_and_outputs"] = peak_above(pk, out_bytes)
        r["torch_peak_bytes_above_inputs_and_outputs"] = peak_above(tc, out_bytes)
        if r["torch_over_package"] < 1:
            r["verdict"] = "TORCH IS FASTER"
        rec["shapes"].append(r)
        print(json.dumps(r), flush=True)
        del rgb, mask, K
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "ops.ingest_views (three launches: box pass, geometry pass, resize pass) on whole sequences against (a) the same "
                               "steps composed from torch ops on the device in chunks of 64 frames, (b) host loops of the rule per frame "
                               "(extrapolated to n frames for the ratios), (c) the byte floor at the copy bandwidth measured in this run, "
                               "(d) its three empty launches.  HIP events around `calls_per_round` calls, per call; one process; the "
                               "repeat-to-repeat spread is min_ms .. max_ms and package_events_again",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "the three kernels apart; hardware counters; reading and decoding the PNG files (PIL, on the host) and "
                                       "the host-to-device copy of the frames, which ingest.generate_bop_realsamples pays per chunk and which "
                                       "dominate a real folder; cv2's own loop (cv2 is absent: unpinned, from memory); Cm = 1 masks",
                       **rec}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
