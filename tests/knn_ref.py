"""Shared by the k-NN and local-frame tests (not a test module): NumPy restatements of csrc/knn.hpp's search (the f32 fmaf
chain of tests/back_march_ref.brute_count, then np.lexsort on (index, d2 bits)) and of its frames (numpy.linalg.eigh for the
vectors, exact rational arithmetic for the sign rule's f64 fma), and the tests' shapes.

`python -m tests.knn_ref` measures, on the CPU, how far the host build's normals and curvatures are from eigh's on the frame
clouds below and writes profiles/knn_normals_parity.json; tests/test_knn_cpu.py allows 100 x those figures."""
import functools
import json
from fractions import Fraction
from pathlib import Path

import numpy as np

from tests import density_ref as dr

f32, f64 = np.float32, np.float64
ROOT = Path(__file__).resolve().parent.parent
MIN_GAP = 1e-3          # every frame cloud keeps (l1 - l0) / l2 above this at every point


def d2_bits(q, t):
    """(Nt,) uint32: the bits of d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in f32, d = t - q."""
    d = (np.asarray(t, f32) - np.asarray(q, f32)).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        d2 = dr.fma32(d[:, 2], d[:, 2], dr.fma32(d[:, 1], d[:, 1], (d[:, 0] * d[:, 0]).astype(f32)))
    return np.ascontiguousarray(d2, f32).view(np.uint32)


def brute_knn(query, target, K):
    """csrc/knn.hpp's rule over every pair -> (idx (Nq,K) int32, d2 (Nq,K) f32): (d2, index) ascending."""
    q, t = np.asarray(query, f32), np.asarray(target, f32)
    idx = np.empty((len(q), K), np.int32)
    d2 = np.empty((len(q), K), f32)
    j = np.arange(len(t))
    for i in range(len(q)):
        bits = d2_bits(q[i], t)
        order = np.lexsort((j, bits))[:K]
        idx[i] = order
        d2[i] = bits[order].view(f32)
    return idx, d2


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (query, target, K): the search tests' shapes.  Arrays are shared: leave them unchanged."""
    rng = np.random.default_rng(17)
    out = {}
    one = np.array([[0.25, -1.0, 3.0]], f32)
    out["Nt = 1, K = 1"] = (rng.uniform(-1, 1, (5, 3)).astype(f32), one, 1)
    cloud = rng.uniform(-0.5, 0.5, (300, 3)).astype(f32)
    out["K = 1"] = (rng.uniform(-0.5, 0.5, (70, 3)).astype(f32), cloud, 1)
    out["K = Nt"] = (cloud[:40], cloud, 300)
    same = np.tile(np.array([[0.1, 0.2, 0.3]], f32), (33, 1))
    out["all identical"] = (same, same, 7)
    lattice = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    out["integer lattice, cut inside the six axis neighbours"] = (lattice, lattice, 4)
    dup = rng.uniform(-0.2, 0.2, (40, 3)).astype(f32)
    dup = np.concatenate([dup, dup[:17], dup[:5], dup[:17]])
    out["duplicated points"] = (dup, dup, 9)
    # targets on a line through the query: squared distances that differ in the lowest mantissa bits only (the first two
    # groups), and over many binades (the third), so that every digit of the d2 bits decides somewhere
    x = np.concatenate([1.0 + np.arange(200) * 2.0 ** -23, 1.5 + np.arange(200) * 2.0 ** -16,
                        10.0 ** rng.uniform(-3, 3, 200)]).astype(f32)
    x = x[rng.permutation(len(x))]
    line = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    origin = np.zeros((1, 3), f32)
    for K in (150, 333, 520):
        out[f"line, low mantissa bits, K = {K}"] = (np.concatenate([origin, line[:3]]), line, K)
    for Nt in (65, 257, 1000):
        t = rng.normal(0, 0.3, (Nt, 3)).astype(f32)
        q = np.concatenate([t[:19], rng.normal(0, 0.3, (18, 3)).astype(f32)])
        for K in sorted({k for k in (1, 2, 63, 64, 65, 400, min(Nt, 1024)) if k <= Nt}):
            out[f"Nt = {Nt}, K = {K}"] = (q, t, K)
    out["queries apart from the targets"] = (rng.uniform(2, 3, (37, 3)).astype(f32), cloud, 50)
    return out


def surface_cloud(kind, n, seed):
    """n points drawn uniformly from the surface of synth.make_mesh(kind) (tests/test_gpu_radius._surface_cloud's way)."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import synth
    rng = np.random.default_rng(seed)
    v, tri = synth.make_mesh("torus", 32, radius=0.5, tube=0.2) if kind == "torus" else synth.make_mesh("sphere", 24, radius=0.5)
    v, tri = np.asarray(v, f64), np.asarray(tri)
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    pick = rng.choice(len(tri), n, p=area / area.sum())
    u, w = rng.uniform(size=n), rng.uniform(size=n)
    flip = u + w > 1
    u[flip], w[flip] = 1 - u[flip], 1 - w[flip]
    return (a[pick] + u[:, None] * (b[pick] - a[pick]) + w[:, None] * (c[pick] - a[pick])).astype(f32)


@functools.lru_cache(maxsize=None)
def frame_clouds():
    """name -> (points, K): the frame tests' shapes; test_knn_cpu checks MIN_GAP on every point of each with eigh alone."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    rng = np.random.default_rng(23)
    plane = np.concatenate([rng.uniform(-1, 1, (400, 2)), rng.normal(0, 0.01, (400, 1))], 1).astype(f32)
    sphere, torus = surface_cloud("sphere", 700, 3), surface_cloud("torus", 900, 4)
    dense = surface_cloud("torus", 6000, 5)
    ref = dense[ops.fps_sample_host(dense, 1000)[0].astype(np.int64)]           # generateCors.py's shape: 1 000 FPS points
    return {"noisy plane, K = 20": (plane, 20), "sphere, K = 20": (sphere, 20), "sphere, K = 50": (sphere, 50),
            "torus, K = 20": (torus, 20), "torus, K = 50": (torus, 50), "1000 FPS points, K = 400": (ref, 400)}


def covariances(points, idx):
    """(N,3,3) f64: the covariance of each row's neighbours about their own mean, divided by K."""
    nb = np.asarray(points, f64)[np.asarray(idx, np.int64)]                   # (N, K, 3)
    d = nb - nb.mean(axis=1, keepdims=True)
    return np.einsum("nka,nkb->nab", d, d) / idx.shape[1]


def eigh_frames(points, idx):
    """numpy.linalg.eigh of the covariances -> (eigenvalues (N,3) ascending, eigenvectors (N,3,3) as columns)."""
    return np.linalg.eigh(covariances(points, idx))


def angle(a, b):
    """The angle between the lines spanned by unit vectors a and b (N,3): asin |a x b|, accurate near 0."""
    return np.arcsin(np.minimum(np.linalg.norm(np.cross(a, b), axis=1), 1.0))


def _fma(a, b, c):
    """f64 fma(a, b, c): the exact rational value rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def positive_counts(points, idx, vec):
    """(N,) int: how many neighbours j of point i have fma(v_z, dz, fma(v_y, dy, v_x dx)) > 0 in f64, d = p_j - p_i, for
    the vectors vec (N,3) — include/isr_knn.h's sign rule, exactly."""
    p = np.asarray(points, f32).astype(f64)
    out = np.zeros(len(p), np.int64)
    for i in range(len(p)):
        vx, vy, vz = (float(c) for c in vec[i])
        for j in idx[i]:
            dx, dy, dz = (float(c) for c in p[j] - p[i])
            out[i] += _fma(vz, dz, _fma(vy, dy, vx * dx)) > 0.0
    return out


def measure_parity():
    """The largest angle between the host normals and eigh's, and the largest curvature difference relative to the largest
    eigenvalue, over every point of every frame cloud."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    rows = {}
    for name, (pts, K) in frame_clouds().items():
        idx = ops.knn_host(pts, pts, K)[0]
        curv, frames = ops.local_frames_host(pts, idx, disambiguate=False)
        w, v = eigh_frames(pts, idx)
        rows[name] = {"points": len(pts), "K": K, "min_relative_gap": float(((w[:, 1] - w[:, 0]) / w[:, 2]).min()),
                      "max_normal_angle_rad": float(angle(frames[:, :, 0], v[:, :, 0]).max()),
                      "max_curvature_diff_rel": float((np.abs(curv - w) / w[:, 2:3]).max())}
    return rows


if __name__ == "__main__":
    rows = measure_parity()
    doc = {"what": "isr_local_frames_host against numpy.linalg.eigh of the same covariances (f64), measured on the CPU by "
                   "python -m tests.knn_ref; tests/test_knn_cpu.py allows 100 x the two maxima",
           "max_normal_angle_rad": max(r["max_normal_angle_rad"] for r in rows.values()),
           "max_curvature_diff_rel": max(r["max_curvature_diff_rel"] for r in rows.values()), "clouds": rows}
    (ROOT / "profiles" / "knn_normals_parity.json").write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))
