"""ops.knn and sampling.estimate_pointcloud_normals on the device, at the two shapes the reference has:
    python tools/bench_knn.py [--out profiles/knn_normals.json] [--reps 5] [--large 80000]
  * (1 000, 1 000, K = 400): generateCors.py:208-211, 1 000 FPS points and their 400 neighbours;
  * (80 000, 80 000, K = 50): the key cloud's size (genFeat.py:199-201).
Each is ops.knn against torch.cdist + topk on the same device (rows in chunks, so that the distance matrix fits) — HIP events,
median and spread over `reps` after one warm-up call — and against sklearn.neighbors.KDTree.query on the CPU (wall clock, one
run at the large shape); estimate_pointcloud_normals (the search, the frames and the f32 conversion) is timed at both.
The clouds are points on a torus.  The neighbour SETS of the three routes are compared where the K-th and (K+1)-th distances
differ; cdist's distances are another arithmetic, so its order inside a row is not compared.
No threshold: the record is the measurement."""
import argparse, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops, sampling
from bench_render import event_timed, stats


def torus_cloud(n, seed):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    r = 0.5 + 0.2 * np.cos(v)
    return np.stack([r * np.cos(u), r * np.sin(u), 0.2 * np.sin(v)], 1).astype(np.float32)


def cdist_topk(q, t, K, rows):
    out = []
    for i in range(0, q.shape[0], rows):
        out.append(torch.cdist(q[i:i + rows], t).topk(K, dim=1, largest=False).indices)
    return torch.cat(out)


def case(n, K, reps, rows, kdtree_reps):
    from sklearn.neighbors import KDTree
    dev = torch.device("cuda:0")
    pts = torus_cloud(n, n)
    t = torch.from_numpy(pts).to(dev)
    ours = lambda: ops.knn(t, t, K, check_finite=False)
    other = lambda: cdist_topk(t, t, K, rows)
    normals = lambda: sampling.estimate_pointcloud_normals(t, K)
    idx, d2 = ours()
    ref = other()
    normals()
    torch.cuda.synchronize()
    t_ours, t_other, t_normals = (stats(event_timed(f, reps)) for f in (ours, other, normals))
    tree_ms = []
    for _ in range(kdtree_reps):
        t0 = time.perf_counter()
        tree_idx = KDTree(pts, leaf_size=2).query(pts, k=K)[1]
        tree_ms.append((time.perf_counter() - t0) * 1e3)
    # rows whose K-th distance stands alone define one neighbour set
    more = ops.knn(t[:2000], t, K + 1, check_finite=False)[1]
    clear = (more[:, K] > more[:, K - 1]).cpu().numpy()
    ours_sets = np.sort(idx[:2000].cpu().numpy(), axis=1)[clear]
    same_cdist = float((ours_sets == np.sort(ref[:2000].cpu().numpy(), axis=1)[clear]).all(axis=1).mean())
    same_tree = float((ours_sets == np.sort(tree_idx[:2000], axis=1)[clear]).all(axis=1).mean())
    return {"Nq": n, "Nt": n, "K": K, "knn_events": t_ours, "cdist_topk_events": t_other, "cdist_rows_per_chunk": rows,
            "cdist_topk_over_knn": round(t_other["median_ms"] / t_ours["median_ms"], 3),
            "kdtree_build_and_query_wall_ms": [round(m, 1) for m in tree_ms],
            "kdtree_over_knn": round(float(np.median(tree_ms)) / t_ours["median_ms"], 3),
            "estimate_pointcloud_normals_events": t_normals,
            "rows_compared": int(clear.sum()), "share_of_rows_with_cdist_topk_set": round(same_cdist, 4),
            "share_of_rows_with_kdtree_set": round(same_tree, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--large", type=int, default=80000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    rows = [case(1000, 400, a.reps, 1000, 3), case(a.large, 50, a.reps, 8192, 1)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "ops.knn against torch.cdist + topk (HIP events, same device) and sklearn's KDTree (CPU, wall clock), "
                               "and estimate_pointcloud_normals, on torus clouds; one process",
                       "device": torch.cuda.get_device_name(0), "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
