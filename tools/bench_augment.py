"""One training batch of trainPose.py's loader on the device (ops.augment_images + ops.augment_rays), timed with HIP events:
    python tools/bench_augment.py [--out profiles/augment.json] [--rounds 7] [--calls 20]
16 images of 224 x 224 with canvases, occluder rectangles, both shifts and border kernels on some; S = 1 024 rays per image
and set from 16 views of about 20 000 rows.  Against
  * the same steps composed from torch on the device: affine_grid / grid_sample three times (the image and the occluded mask
    by M + tra1, the original mask by M + tra), the integer shift by slicing, where, max_pool2d for the dilation, normalize; per
    image and set mm, the subtraction, a boolean mask and randperm — its numbers differ (f32 sampling, another random
    stream): it is the same work, not the same bytes;
  * the launch floor: as many one-element fills as the package launches kernels (two for the images, one for the rays);
  * the byte floor: every input the call must read once and every output written once, at 6.3 TB/s.
A round is `calls` calls between two events, after one warm-up call of every route; the record holds the median, the fastest
and the slowest round per call, whether two calls give identical bytes, and the peak memory above the inputs.  No threshold:
the record is the measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import augment, ops
from tests import augment_ref as ar

HBM_BYTES_PER_S = 6.3e12
B, H, S, ROWS = 16, 224, 1024, 20000


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


def inputs(dev):
    rng = np.random.default_rng(0)
    rgb, mask, orig, canvas = ar.image_inputs(rng, B, H, H)
    mask[:] = 0
    mask[:, 40:180, 50:170] = 1
    p = augment.draw_params(B, 3, H, bbox=np.array([[50, 40, 120, 140]] * B), integral=augment.mask_integral(torch.from_numpy(mask)),
                            borderADD=True, maskMax=100, scaleFac=0.8)
    rows = [rng.uniform(-0.8, 0.8, (ROWS + 37 * v, 2)).astype(np.float32) for v in range(B)]
    front, back = ar.ray_bank(rng, rows), ar.ray_bank(rng, rows[::-1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(rgb=t(rgb), mask=t(mask), canvas=t(canvas), p=p, front=(t(front[0]), t(front[1]), front[2]),
                back=(t(back[0]), t(back[1]), back[2]), ids=np.arange(B))


def package_route(d):
    p = d["p"]
    M, rect, tra, tra1, border = p.M.numpy(), p.rect.numpy(), p.tra.numpy(), p.tra1.numpy(), p.border.numpy()
    rot, t = p.ray_rot.numpy(), p.ray_t.numpy()

    def images():
        return ops.augment_images(d["rgb"], d["mask"], M, canvas=d["canvas"], rect=rect, tra=tra, tra1=tra1, border=border)

    def rays():
        return ops.augment_rays(d["front"], d["ids"], rot, t, S, 11, back=d["back"])

    return images, rays


def torch_route(d, dev):
    p = d["p"]
    mu, sd = torch.tensor(ops.IMAGENET_MEAN, device=dev), torch.tensor(ops.IMAGENET_STD, device=dev)

    def theta(t):      # tests/test_augment_cpu.grid_sample_warp's matrix, H = W
        out = np.zeros((B, 2, 3), np.float32)
        for b in range(B):
            inv = ar.invert(p.M[b].numpy(), t[b])
            out[b] = [[inv[0], inv[1], (inv[0] * (H - 1) + inv[1] * (H - 1) + 2 * inv[2] + 1) / H - 1],
                      [inv[3], inv[4], (inv[3] * (H - 1) + inv[4] * (H - 1) + 2 * inv[5] + 1) / H - 1]]
        return torch.from_numpy(out).to(dev)

    th1, th2 = theta(p.tra1.numpy()), theta(p.tra.numpy())
    d_xy = (p.tra - p.tra1).tolist()
    rect, border = p.rect.tolist(), p.border.tolist()
    rot, tt = torch.from_numpy(p.ray_rot.numpy().reshape(B, 2, 2)).to(dev), torch.from_numpy(p.ray_t.numpy()).to(dev)
    gs = lambda x, th: torch.nn.functional.grid_sample(x, torch.nn.functional.affine_grid(th, x.shape, align_corners=False),
                                                       mode="bilinear", padding_mode="zeros", align_corners=False)

    def shift(x, dx, dy):
        out = torch.zeros_like(x)
        xs0, xs1, ys0, ys1 = max(dx, 0), min(H + dx, H), max(dy, 0), min(H + dy, H)
        if xs1 > xs0 and ys1 > ys0:
            out[..., ys0:ys1, xs0:xs1] = x[..., ys0 - dy:ys1 - dy, xs0 - dx:xs1 - dx]
        return out

    def images():
        m = d["mask"].to(torch.float32)
        occ = m.clone()
        for b, (x, y, w, h) in enumerate(rect):
            if w > 0 and h > 0:
                occ[b, y:y + h, x:x + w] = 0
        first = gs(d["rgb"].permute(0, 3, 1, 2), th1)
        first_mask = gs(occ[:, None], th1).round()
        orig = gs(m[:, None], th2).round()[:, 0]
        dst = torch.stack([shift(first[b], *d_xy[b]) for b in range(B)])
        dst_mask = torch.stack([shift(first_mask[b], *d_xy[b]) for b in range(B)])
        out = torch.where(dst_mask == 1, dst, d["canvas"].permute(0, 3, 1, 2))
        for b, (kh, kw) in enumerate(border):
            if kh > 0 and kw > 0:
                dil = torch.nn.functional.max_pool2d(torch.nn.functional.pad(dst_mask[b:b + 1], (kw // 2, kw - 1 - kw // 2, kh // 2, kh - 1 - kh // 2)),
                                                     (kh, kw), stride=1)
                out[b] = torch.where(dil[0] <= 0.9, torch.zeros_like(out[b]), out[b])
        out = (out.permute(0, 2, 3, 1) - mu) / sd
        return out, orig, dst_mask[:, 0]

    def rays():
        res = []
        for bank in (d["front"], d["back"]):
            for b in range(B):
                lo, hi = int(bank[2][b]), int(bank[2][b + 1])
                s = torch.mm(bank[0][lo:hi], rot[b].T) - tt[b]
                idx = torch.where((s[:, 0] > -1) & (s[:, 0] < 1) & (s[:, 1] > -1) & (s[:, 1] < 1))[0]      # the filter, always: no host read of max / min
                samps = idx[torch.randperm(idx.shape[0], device=dev)[:S]]
                res.append((s[samps], bank[1][lo:hi][samps]))
        return res

    return images, rays


def tensors(r):
    if isinstance(r, torch.Tensor):
        return [r]
    if hasattr(r, "xys"):
        return [r.xys, r.pos, r.index, r.count]
    return [x for item in r for x in tensors(item)]


def identical(fn):
    a, b = [x.clone() for x in tensors(fn())], [x.clone() for x in tensors(fn())]
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    del r
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    d = inputs(dev)
    p_img, p_rays = package_route(d)
    t_img, t_rays = torch_route(d, dev)
    one = torch.empty(1, dtype=torch.int32, device=dev)
    rows_total = int(d["front"][2][-1] + d["back"][2][-1])
    rec = {"shape": {"B": B, "H": H, "W": H, "S": S, "rows_per_view": f"{ROWS}..{ROWS + 37 * (B - 1)}", "sets": 2,
                     "images_with_a_rectangle": int((d["p"].rect[:, 2] > 0).sum()), "images_with_a_border_kernel": int((d["p"].border[:, 0] > 0).sum())}}
    for name, pk, tc, launches, nbytes in (
            ("images", p_img, t_img, 2, B * H * H * (12 + 1 + 12) + B * H * H * 4 * 5),           # rgb, mask, canvas read; 5 f32 written
            ("rays", p_rays, t_rays, 1, rows_total * 8 + 2 * B * S * (8 + 12 + 4))):                # every location read once; the sample written
        r = {"kernel_launches": launches}
        r["package_events"] = timed(pk, a.rounds, a.calls)
        r["torch_events"] = timed(tc, a.rounds, max(a.calls // 4, 2))
        r["launch_floor_fills_events"] = timed(lambda: [one.fill_(1) for _ in range(launches)], a.rounds, a.calls)
        r["package_events_again"] = timed(pk, a.rounds, a.calls)
        r["byte_floor_ms"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 5)
        ms = r["package_events"]["median_ms"]
        r["torch_over_package"] = round(r["torch_events"]["median_ms"] / ms, 3)
        r["package_over_launch_floor"] = round(ms / r["launch_floor_fills_events"]["median_ms"], 2)
        r["package_over_byte_floor"] = round(ms / r["byte_floor_ms"], 2)
        r["package_two_calls_identical_bytes"] = identical(pk)
        r["torch_two_calls_identical_bytes"] = identical(tc)
        r["package_peak_bytes_above_inputs"] = peak(pk)
        r["torch_peak_bytes_above_inputs"] = peak(tc)
        if r["torch_over_package"] < 1:
            r["verdict"] = "TORCH IS FASTER"
        rec[name] = r
        print(json.dumps({name: r}), flush=True)
    both = lambda: (p_img(), p_rays())
    rec["batch_package_events"] = timed(both, a.rounds, a.calls)
    rec["batch_torch_events"] = timed(lambda: (t_img(), t_rays()), a.rounds, max(a.calls // 4, 2))
    print(json.dumps({k: rec[k] for k in ("batch_package_events", "batch_torch_events")}), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "ops.augment_images + ops.augment_rays on one training batch of trainPose.py's shape against the same steps "
                               "composed from torch on the device, the launch floor (one-element fills, one per kernel launch) and the "
                               "byte floor (inputs read once, outputs written once, 6.3 TB/s).  HIP events around `calls_per_round` "
                               "calls, per call; one process; the repeat-to-repeat spread is min_ms .. max_ms and package_events_again",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "the two image kernels apart; hardware counters; the host's parameter draw (augment.draw_params); "
                                       "the gather of the batch's views from the resident set (torch indexing in augment.PoseBatches); "
                                       "the reference's own loader (cv2 and albumentations are absent)",
                       **rec}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
