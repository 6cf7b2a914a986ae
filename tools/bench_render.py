"""The object-coordinate renderer (render.ObjCoordRenderer, isr_render_coords_batch) at the reference's crop shape:
    python tools/bench_render.py [--out profiles/render_coords.json] [--reps 20]
For meshes of about 2 000, 20 000 and 200 000 faces (torus) at 224 x 224: render_batch with B = 1 and B = 32, timed with HIP
events around the call after a warm-up (device time of the three launches; the median and the min-max spread over `reps`),
against the same 32 images from 32 single render() calls (host clock, device-synchronised: each call ends in the copy of its
image to the host, as refine_pose uses it).  Then the render's share of a sequence.estimate_and_refine block (B = 32,
optimizer="device") whose renderer is this one: the block's wall time and, from ops' event timers inside the same runs, the
time of its one isr_render_coords_batch call.  No threshold: the record is the measurement."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops, render, sequence, synth

RES = 224


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "rounds": len(ms)}


def event_timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


class Field:
    def __init__(self, W):
        self.W = W

    def batched_customForward(self, x):
        f = torch.sin(x @ self.W.to(x.device))
        return torch.cat([f, torch.ones(len(x), 1, device=x.device)], dim=-1)


def surf_block(B, e, rng, dev, n=142):
    """A torus (about 20 000 faces) seen in B crops: mask logits from the renderer, query pixels carrying the keys of the
    vertices that land there."""
    radius, tube = 32.0, 0.4
    v, f = synth.make_mesh("torus", n, radius=radius, tube=tube)
    ring = v.copy()
    ring[:, 2] = 0
    ring *= radius / np.linalg.norm(ring, axis=1, keepdims=True)
    nrm = (v - ring) / (radius * tube)
    keys = synth.unit_keys(rng, len(v), e, tau=6.0)
    obj = render.Mesh(v, f)
    rend = render.ObjCoordRenderer([obj], RES)
    K = np.array([[930.0, 0, RES / 2 - 0.5], [0, 930.0, RES / 2 - 0.5], [0, 0, 1]])
    Rg, tg = synth.random_poses(rng, B, tz=420.0, t_sigma=5.0)
    mls, qs = [], []
    for b in range(B):
        img = rend.render(0, K, Rg[b], tg[b][:, None])
        depth = rend.read_depth()
        uv = synth.project(K, Rg[b], tg[b], v)
        cam = v @ Rg[b].T + tg[b]
        ui, vi = np.rint(uv[:, 0]).astype(int), np.rint(uv[:, 1]).astype(int)
        ok = np.nonzero((ui >= 0) & (ui < RES) & (vi >= 0) & (vi < RES) & ((nrm @ Rg[b].T * cam).sum(1) < 0))[0]
        ok = ok[np.abs(depth[vi[ok], ui[ok]] - cam[ok, 2]) < 2.0]
        qq = (0.3 * rng.normal(size=(RES, RES, e))).astype(np.float32)
        qq[vi[ok], ui[ok]] = keys[ok] + 0.2 * rng.normal(size=(len(ok), e)).astype(np.float32)
        mls.append(np.where(img[..., 3] == 1, 6.0, -6.0).astype(np.float32))
        qs.append(qq)
    field = Field(torch.from_numpy(rng.normal(0, 2.0, (3, e)).astype(np.float32)))
    kv = field.batched_customForward(torch.from_numpy((v * 1.8 / obj.diameter).astype(np.float32)).to(dev))[:, :e].float()
    return dict(v=v, nrm=nrm, keys=keys, obj=obj, rend=rend, K=K, Rg=Rg, tg=tg, field=field, kv=kv,
                ml=torch.from_numpy(np.stack(mls)).to(dev), q=torch.from_numpy(np.stack(qs)).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--block-reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(9)
    K = np.array([[448.0, 0, RES / 2 - 0.5], [0, 448.0, RES / 2 - 0.5], [0, 0, 1]])
    Rs, ts = synth.random_poses(rng, 32, tz=420.0, t_sigma=8.0)
    rows = []
    for n in (45, 142, 450):
        v, f = synth.make_mesh("torus", n)
        rend = render.ObjCoordRenderer([render.Mesh(v, f)], RES)
        row = {"faces": len(f), "res": RES}
        for B in (1, 32):
            Rb, tb = list(Rs[:B]), list(ts[:B])
            batch = lambda: rend.render_batch(0, K, Rb, tb)
            batch()
            torch.cuda.synchronize()
            # the pose upload is part of the wrapper; time the C call alone as well, on cameras already on the device
            Kd, Rtd = rend._cameras(K, Rb, tb)
            call = lambda: rend._draw(0, Kd, Rtd, True, None)
            call()
            row[f"batch_B{B}_call_events"] = stats(event_timed(call, a.reps))
            row[f"batch_B{B}_events"] = stats(event_timed(batch, a.reps))
        imgs = rend.render_batch(0, K, list(Rs), list(ts)).cpu().numpy()
        loop_ms = []
        for _ in range(max(3, a.reps // 4)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            singles = [rend.render(0, K, Rs[b], ts[b][:, None]) for b in range(32)]
            torch.cuda.synchronize()
            loop_ms.append((time.perf_counter() - t0) * 1e3)
        assert all(singles[b].tobytes() == imgs[b].tobytes() for b in range(32)), "batch and single renders disagree"
        row["loop_32_single_wall"] = stats(loop_ms)
        row["covered_px_mean"] = float((imgs[..., 3] == 1).sum() / 32)
        rows.append(row)
        print(json.dumps(row), flush=True)
    # the render's share of a useSurfEval block
    B, e = 32, 12
    s = surf_block(B, e, rng, dev)
    pts_d, keys_d = torch.from_numpy(s["v"].astype(np.float32)).to(dev), torch.from_numpy(s["keys"]).to(dev)
    args = (s["ml"], s["q"], pts_d, s["nrm"], keys_d, synth.diameter(s["v"]), s["K"], s["rend"], 0, s["obj"], s["field"], s["kv"],
            s["v"][::10], s["Rg"], s["tg"])
    kw = dict(estimate_kw=dict(max_pose_evaluations=1000), refine_kw=dict(optimizer="device"))
    sequence.estimate_and_refine(*args, **kw)
    block_ms, render_ms, refined = [], [], 0
    for _ in range(a.block_reps):
        ops.enable_timing(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sequence.estimate_and_refine(*args, **kw)
        torch.cuda.synchronize()
        block_ms.append((time.perf_counter() - t0) * 1e3)
        rec = ops.drain_timing()
        ops.enable_timing(False)
        assert rec["render_coords"][0] == 1
        render_ms.append(rec["render_coords"][1])
        refined = int(out["refined"].sum())
    share = {"B": B, "faces": int(len(s["obj"].mesh.faces)), "refined": refined, "block_wall": stats(block_ms),
             "render_call_events": stats(render_ms),
             "render_share_of_block": round(statistics.median(render_ms) / statistics.median(block_ms), 5),
             "note": "wall time of the block with event timers on; the render is one isr_render_coords_batch call"}
    print(json.dumps(share), flush=True)
    doc = {"what": "ObjCoordRenderer.render_batch (HIP events) against 32 single render() calls (wall), torus meshes, 224 x 224",
           "device": torch.cuda.get_device_name(0), "rows": rows, "estimate_and_refine_share": share}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
