"""One generateCors.py view on the device (correspondences.view_correspondences) and its parts:
    python tools/bench_correspondences.py [--out profiles/view_correspondences.json] [--reps 5] [--rays 50176] [--points 256]
H = 60, 360 -> 256 -> 256 -> 1, Softplus(10); 50 176 rays x 256 points; the mesh is key_export.extract_mesh of the same field.
  * the back march in threshold mode (tiles in front of a ray's last hit skipped) against the same rays with every density
    asked for (every point evaluated) — HIP events, median and spread over `reps` after one warm-up call;
  * ops.radius_count on the mesh vertices (radius 0.05, cap 21: generateCors.py:257's clean-up) — HIP events;
  * view_correspondences against the same steps with the field as a torch module in 16 chunks, torch's march
    (tests/density_ref.torch_march and tests/back_march_ref.torch_march_back) and sklearn's KDTree — wall clock around a
    synchronise, both routes cross the host for the mesh distances.
No threshold: the record is the measurement."""
import argparse, json, os, sys, time
from types import SimpleNamespace
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import correspondences, key_export, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
from bench_render import event_timed, stats
from tests.back_march_ref import torch_march_back
from tests.density_ref import TorchDensity, fixture, frequencies, torch_march


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(out)), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "n": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rays", type=int, default=224 * 224)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--res", type=int, default=128)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    from sklearn.neighbors import KDTree
    dev = torch.device("cuda:0")
    H, hidden = 60, 256
    Ws, bs = fixture(H, hidden, 2, seed=5)
    field = DensityField(Ws, bs, frequencies(H), 10.0, dev)
    module = TorchDensity(Ws, bs, frequencies(H)).to(dev)
    rng = np.random.default_rng(5)
    N, P = a.rays, a.points
    o = rng.normal(size=(N, 3)).astype(np.float32)
    o *= 2.5 / np.linalg.norm(o, axis=1, keepdims=True)
    d = -o / np.linalg.norm(o, axis=1, keepdims=True) + rng.normal(0, 0.15, (N, 3)).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    ln = np.tile(np.linspace(1.0, 4.0, P).astype(np.float32), (N, 1))
    xys = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
    to, td, tl, txy = (torch.from_numpy(x).to(dev) for x in (o, d, ln, xys))
    rays = SimpleNamespace(origins=to[None], directions=td[None], lengths=tl[None], xys=txy[None])

    verts = np.asarray(key_export.extract_mesh(field, res=a.res).mesh.vertices)
    tv = torch.from_numpy(verts.astype(np.float32)).to(dev)
    t_count = stats(event_timed(lambda: ops.radius_count(tv, 0.05, 21, check_finite=False), a.reps))
    clean, ind = correspondences.clean_mesh_vertices(verts, 20, 0.05)
    if len(clean) == 0:
        clean = verts

    back = lambda dens: ops.density_march(field.pack, field.widths, field.H, to, td, tl, 0.05, want_densities=dens, direction="back")
    got_skip, got_full = back(False), back(True)
    torch.cuda.synchronize()
    same = bool(torch.equal(got_skip[1].view(torch.int32), got_full[1].view(torch.int32)))
    rho = got_full[3]
    above = rho > 0.05
    last = torch.where(above.any(1), (P - 1 - above.flip(1).float().argmax(1)), torch.full((N,), -1, device=dev))
    tiles_total = (P + 63) // 64
    tiles_walked = torch.where(last >= 0, tiles_total - last // 64, torch.full_like(last, tiles_total)).float().mean()
    t_skip = stats(event_timed(lambda: back(False), a.reps))
    t_full = stats(event_timed(lambda: back(True), a.reps))

    def ours():
        return correspondences.view_correspondences(field, rays, clean)

    tree = KDTree(np.asarray(clean), leaf_size=2)

    def dens(o_, d_, l_):
        pts = (o_[:, None, :] + d_[:, None, :] * l_[:, :, None]).reshape(-1, 3)
        return torch.cat([module(c)[..., 0] for c in torch.chunk(pts, 16)]).view(l_.shape)

    def reference_route():
        _, depth = torch_march(dens(to, td, tl), tl, 0.2)
        pos = (to + td * depth[:, None]).cpu()
        dist, _ = tree.query(pos.numpy(), k=1)
        idx1 = np.where(dist[:, 0] < 0.1)[0]
        pos = pos[idx1].to(dev)
        o1, l1 = to[idx1], tl[idx1]
        bd = -(o1 / torch.norm(o1, dim=-1).unsqueeze(-1))
        bl = (l1 - l1[:, :1]) / 3
        if len(idx1) == 0:
            return pos, pos
        _, bdepth = torch_march_back(dens(pos, bd, bl), bl, 0.05)
        posb = (pos + bd * bdepth[:, None]).cpu()
        dist2, _ = tree.query(posb.numpy(), k=1)
        return pos, posb[np.where(dist2[:, 0] < 0.1)[0]]

    vc = ours()
    ref = reference_route()
    t_ours = wall(ours, a.reps)
    t_ref = wall(reference_route, a.reps)
    row = {"rays": N, "points_per_ray": P, "H": H, "hidden": [hidden, hidden], "mesh_res": a.res, "mesh_vertices": int(len(verts)),
           "mesh_vertices_kept": int(len(ind)),
           "share_of_points_above_0.05": round(float(above.float().mean()), 4),
           "mean_tiles_walked_by_the_threshold_back_march": round(float(tiles_walked), 3), "tiles_per_ray": tiles_total,
           "back_march_threshold_events": t_skip, "back_march_every_point_events": t_full,
           "every_point_over_threshold": round(t_full["median_ms"] / t_skip["median_ms"], 3),
           "threshold_and_every_point_depths_equal": same,
           "radius_count_on_mesh_vertices_events": t_count,
           "view_correspondences_wall": t_ours, "torch_march_and_kdtree_wall": t_ref,
           "torch_over_view_correspondences": round(t_ref["median_ms"] / t_ours["median_ms"], 3),
           "n1": int(vc.pos_vec.shape[1]), "n2": int(vc.pos_vec_back.shape[1]),
           "n1_torch_route": int(ref[0].shape[0]), "n2_torch_route": int(ref[1].shape[0])}
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "one generateCors.py view: the back march with and without the tile skip, the radius count of the "
                               "mesh clean-up, and view_correspondences against torch's march and sklearn's KDTree; one process, "
                               "same inputs", "device": torch.cuda.get_device_name(0), "view": row}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
