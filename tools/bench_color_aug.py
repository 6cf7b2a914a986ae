"""The colour augmentation pass (ops.augment_color) at trainPose.py's shape, 16 x 224 x 224, timed with HIP events:
    python tools/bench_color_aug.py [--out profiles/color_aug.json] [--rounds 7] [--calls 20]
  * pass 1 (select = the mask, under = the canvas), pass 2 (the border and normalize tail) and both, with every gate forced
    on and with gates drawn by augment.draw_color_params at its defaults;
  * every stage alone (one gate on in every image): which stage bounds the all-on figure;
  * the launch floor: as many one-element fills as a pass with every stage launches kernels (eight);
  * the byte floor: the image read once and written once at the copy bandwidth measured in the same run (a device-to-device
    copy of the same bytes);
  * the host build on one thread per image (B = 1 calls), a stand-in for what a loader worker pays; cv2's and albumentations'
    own time is unmeasured (neither is installed);
  * tools/bench_augment.py's batch (ops.augment_images + ops.augment_rays) in the same session: the rest of the batch
    preparation;
  * whether two calls give identical bytes.
A round is `calls` calls between two events, after one warm-up call; the record holds the median, the fastest and the slowest
round per call.  No threshold: the record is the measurement."""
import argparse, importlib.util, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import augment, ops
from tests import color_aug_ref as cr

B, H = 16, 224


def load_bench_augment():
    spec = importlib.util.spec_from_file_location("bench_augment", os.path.join(ROOT, "tools", "bench_augment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    ba = load_bench_augment()
    timed = lambda fn, calls=a.calls: ba.timed(fn, a.rounds, calls)
    rng = np.random.default_rng(0)
    x_host = cr.image(rng, B, H, H)
    x, canvas = torch.from_numpy(x_host).to(dev), torch.from_numpy(cr.image(rng, B, H, H)).to(dev)
    mask = torch.zeros((B, H, H), device=dev)
    mask[:, 40:180, 50:170] = 1
    border = np.tile([[7, 5]], (B, 1))
    forced = (cr.all_on(rng, B), cr.all_on(rng, B))
    drawn = tuple(augment.draw_color_params(B, s).programs() for s in (1, 2))
    pass1 = lambda p: ops.augment_color(x, p[0], select=mask, under=canvas)
    pass2 = lambda p, src=x: ops.augment_color(src, p[1], border=border, border_mask=mask, mean=ops.IMAGENET_MEAN, std=ops.IMAGENET_STD)
    both = lambda p: pass2(p, pass1(p))
    rec = {"shape": {"B": B, "H": H, "W": H}, "geometry": ops.color_aug_geometry(),
           "drawn_gates_on": {g: [int((q[g] > 0).sum()) for q in drawn] for g in ("pass", "jitter", "rbc", "ksize", "iso", "clahe")}}
    for gates, p in (("all_gates_on", forced), ("drawn_gates", drawn)):
        rec[gates] = {"pass1": timed(lambda: pass1(p)), "pass2": timed(lambda: pass2(p)), "both": timed(lambda: both(p)),
                      "both_again": timed(lambda: both(p))}
        print(json.dumps({gates: rec[gates]}), flush=True)
    rec["stage_alone"] = {}
    for gate in ("none", "jitter", "rbc", "blur", "iso", "clahe"):
        p = cr.all_on(np.random.default_rng(5), B, (gate,))
        rec["stage_alone"][gate] = timed(lambda: ops.augment_color(x, p))
    off = ops.color_programs(B)
    rec["stage_alone"]["pass_gate_off_copy"] = timed(lambda: ops.augment_color(x, off))
    print(json.dumps({"stage_alone": rec["stage_alone"]}), flush=True)
    one, dst = torch.empty(1, dtype=torch.int32, device=dev), torch.empty_like(x)
    rec["launch_floor_one_fill"] = timed(lambda: one.fill_(1))
    rec["copy_same_bytes"] = timed(lambda: dst.copy_(x))
    nbytes = 2 * x.numel() * 4
    gbps = nbytes / (rec["copy_same_bytes"]["median_ms"] * 1e-3) / 1e9
    rec["copy_bandwidth_GB_per_s"] = round(gbps, 1)
    rec["byte_floor_ms_per_pass"] = rec["copy_same_bytes"]["median_ms"]
    a_on = rec["all_gates_on"]["both"]["median_ms"]
    launches = rec["geometry"]["max_launches"]
    rec["launch_floor_fills_per_pass"] = timed(lambda: [one.fill_(1) for _ in range(launches)])
    rec["both_all_on_over_launch_floor"] = round(a_on / (2 * rec["launch_floor_fills_per_pass"]["median_ms"]), 1)
    rec["both_all_on_over_byte_floor"] = round(a_on / (2 * rec["byte_floor_ms_per_pass"]), 1)
    first, second = both(forced).clone(), both(forced).clone()
    rec["two_calls_identical_bytes"] = bool(torch.equal(first.view(torch.int32), second.view(torch.int32)))
    ms = []
    for b in range(4):
        t0 = time.perf_counter()
        ops.augment_color_host(x_host[b:b + 1], forced[0][b:b + 1])
        ms.append((time.perf_counter() - t0) * 1e3)
    rec["host_one_thread_ms_per_image_per_pass_all_on"] = {"median": round(statistics.median(ms), 2), "min": round(min(ms), 2), "max": round(max(ms), 2)}
    d = ba.inputs(dev)
    p_img, p_rays = ba.package_route(d)
    rec["bench_augment_batch_same_session"] = timed(lambda: (p_img(), p_rays()))
    rest = rec["bench_augment_batch_same_session"]["median_ms"]
    rec["both_over_rest_of_batch"] = {"all_gates_on": round(a_on / rest, 2), "drawn_gates": round(rec["drawn_gates"]["both"]["median_ms"] / rest, 2)}
    print(json.dumps({k: v for k, v in rec.items() if k not in ("all_gates_on", "drawn_gates", "stage_alone")}), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "ops.augment_color on one training batch of trainPose.py's shape: the two passes of augment.PoseBatches(color=True) "
                               "apart and together, every stage alone, the launch floor (a one-element fill per kernel launch), the byte floor "
                               "(a device-to-device copy of the image's bytes in the same run), the host build on one thread, and "
                               "tools/bench_augment.py's batch in the same session.  HIP events around `calls_per_round` calls, per call; one "
                               "process; the repeat-to-repeat spread is min_ms .. max_ms and both_again",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "cv2's and albumentations' own time (neither is installed); hardware counters; the host's draw "
                                       "(augment.draw_color_params)",
                       **rec}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
