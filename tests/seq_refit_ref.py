"""The sequence-level pose (include/isr_seq_refit.h, csrc/seq_refit.hpp) restated in NumPy: shared by the CPU and GPU tests,
not a test module.

`sums(..., dtype)` is the rule of one pass in plain array arithmetic — no fma, sums by np.sum — in f64 or, as its own
yardstick, in np.longdouble; `solve` is the loop on top of it (np.linalg.solve, the quaternion update); `scene` makes the
seeded synthetic sequences the tests run on."""
import json
import os
from pathlib import Path

import numpy as np

KERNELS = ("l2", "huber", "tukey")
STATUS = ("converged", "max_iter", "few rows", "singular")
PARITY_MARGIN = 4.0          # the project's standing bound: x the f64 restatement's own deviation from its longdouble twin
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 600)         # cap and counts at the tree, wave and block edges
K_DEFAULT = np.array([[500.0, 0.0, 320.0], [0.0, 498.0, 240.0], [0.0, 0.0, 1.0]])
PARITY_FILE = Path(__file__).resolve().parent.parent / "profiles" / "seq_refit_parity.json"


def rot(axis_angle):
    """Rodrigues."""
    v = np.asarray(axis_angle, np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def random_rot(rng, max_deg=180.0):
    v = rng.normal(size=3)
    return rot(v / np.linalg.norm(v) * np.deg2rad(rng.uniform(0, max_deg)))


def weight(kernel, k, a):
    if kernel == "huber":
        return np.where(a <= k, 1.0, k / np.where(a > 0, a, 1))
    if kernel == "tukey":
        q = a / k
        return np.where(a <= k, (1 - q * q) ** 2, 0 * a)
    return np.ones_like(a)


def rows(p3d, p2d, counts, K, G, Y, frame_w=None, kernel="tukey", k=6.0, dtype=np.float64):
    """Every slot's residual r (n, cap, 2), Jacobian J (n, cap, 2, 6), weight w (n, cap) and whether it counts (n, cap)."""
    n, cap = p3d.shape[:2]
    t = dtype
    p, u = p3d.astype(t), p2d.astype(t)
    Km, Gm, Ym = K.reshape(n, 3, 3).astype(t), G.reshape(n, 3, 4).astype(t), np.asarray(Y).astype(t)
    fw = np.ones(n, t) if frame_w is None else np.asarray(frame_w).astype(t)
    with np.errstate(all="ignore"):
        q = p @ Ym[:3, :3].T + Ym[:3, 3]
        c = np.einsum("nab,nmb->nma", Gm[:, :, :3], q) + Gm[:, None, :, 3]
        h = np.einsum("nab,nmb->nma", Km, c)
        pr = h[..., :2] / h[..., 2:3]
        r = pr - u
        rr = (r * r).sum(-1)
        a = np.sqrt(rr)
        w = fw[:, None] * weight(kernel, t(k), a)
        D = (Km[:, None, :2, :] - pr[..., None] * Km[:, None, 2:3, :]) / h[..., 2][..., None, None]      # (n, cap, 2, 3)
        g = np.einsum("nmeb,nbc->nmec", D, Gm[:, :, :3])
        J = np.concatenate([np.cross(q[:, :, None, :], g), g], axis=-1)
        real = np.arange(cap)[None, :] < np.clip(np.asarray(counts), 0, cap)[:, None]
        ok = real & (c[..., 2] > 0) & np.isfinite(rr) & np.isfinite(w) & np.isfinite(J).all((-1, -2)) & (w > 0)
    return r, J, w, ok


def sums(p3d, p2d, counts, K, G, Y, frame_w=None, kernel="tukey", k=6.0, dtype=np.float64):
    """One pass -> dict(a, rr, rows, A (6, 6), b (6,), wrr, frame_stats (n, 4)) in `dtype`."""
    r, J, w, ok = rows(p3d, p2d, counts, K, G, Y, frame_w, kernel, k, dtype)
    z = dtype(0)
    r, J, w = np.where(ok[..., None], r, z), np.where(ok[..., None, None], J, z), np.where(ok, w, z)
    rr = (r * r).sum(-1)
    A = np.einsum("nm,nmei,nmej->nmij", w, J, J).reshape(-1, 6, 6).sum(0)
    b = np.einsum("nm,nmei,nme->nmi", w, J, r).reshape(-1, 6).sum(0)
    stats = np.stack([ok.sum(1).astype(dtype), w.sum(1), (w * rr).sum(1), rr.sum(1)], 1)
    # the sums of the terms' magnitudes: what a sum's rounding error scales with, however much of it cancels
    A_abs = np.abs(np.einsum("nm,nmei,nmej->nmeij", w, J, J)).reshape(-1, 6, 6).sum(0)
    b_abs = np.abs(np.einsum("nm,nmei,nme->nmei", w, J, r)).reshape(-1, 6).sum(0)
    return dict(a=np.sqrt(rr).sum(), rr=rr.sum(), rows=int(ok.sum()), A=A, b=b, wrr=(w * rr).sum(), frame_stats=stats,
                A_abs=A_abs, b_abs=b_abs)


def deviation(x, ld):
    """The largest deviation of the 30 real-valued sums of `x` from the longdouble restatement `ld`, each in units of the sum of
    its terms' magnitudes (for sum a, sum r.r and sum w r.r that is the sum itself).  A sum's rounding error scales with that
    magnitude, not with the sum: b cancels to nothing near the optimum.  One figure over the whole system, because the
    largest of a handful of roundings is a noisy yardstick: over b's 6 entries alone the f64 restatement's own deviation
    ranges over two decades from scene to scene."""
    d = [np.abs(x["A"] - ld["A"]) / ld["A_abs"], np.abs(x["b"] - ld["b"]) / ld["b_abs"]]
    d += [np.atleast_1d(abs(x[q] - ld[q]) / ld[q]) for q in ("a", "rr", "wrr")]
    return float(max(np.max(v) for v in d))


def unpack(v):
    """The entry's 31 sums -> the dict of `sums` (A symmetric)."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = v[3:24]
    A = A + np.triu(A, 1).T
    return dict(a=v[0], rr=v[1], rows=int(v[2]), A=A, b=v[24:30].copy(), wrr=v[30])


def gradient(p3d, p2d, counts, K, G, Y, frame_w=None, kernel="tukey", k=6.0):
    """|J^T W r|, the first-order optimality measure of the iteration's fixed point."""
    return float(np.linalg.norm(sums(p3d, p2d, counts, K, G, Y, frame_w, kernel, k)["b"]))


def step(x):
    """dT(x): the unit quaternion of (1, x0/2, x1/2, x2/2) and the translation x3..5 (icp_plane.hpp's compose)."""
    qv = np.array([1.0, x[0] / 2, x[1] / 2, x[2] / 2])
    qw, qx, qy, qz = qv / np.linalg.norm(qv)
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    return pose(R, x[3:6])


def solve(p3d, p2d, counts, K, G, Y0, frame_w=None, kernel="tukey", k=6.0, max_iter=30, tol_r=1e-10, tol_t=1e-8):
    """The loop in f64 -> (Y, status, passes)."""
    Y = np.array(Y0, np.float64)
    for it in range(max_iter + 1):
        s = sums(p3d, p2d, counts, K, G, Y, frame_w, kernel, k)
        x = None
        if s["rows"] >= 6:
            try:
                x = np.linalg.solve(s["A"], -s["b"])
                if not np.all(np.isfinite(x)) or np.any(np.linalg.eigvalsh(s["A"]) <= 0):
                    x = None
            except np.linalg.LinAlgError:
                x = None
        if x is not None and np.abs(x[:3]).max() < tol_r and np.abs(x[3:]).max() < tol_t:
            return Y, 0, it
        if s["rows"] < 6:
            return Y, 2, it
        if it >= max_iter:
            return Y, 1, it
        if x is None:
            return Y, 3, it
        Y = step(x) @ Y
    raise AssertionError("unreachable")


def pose_error(Y, Y_true):
    """(rotation error in degrees, translation error in mm)."""
    dR = Y[:3, :3] @ Y_true[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    return float(ang), float(np.linalg.norm(Y[:3, 3] - Y_true[:3, 3]))


def scene(seed, n=6, m=60, cap=None, noise=0.5, outliers=0.25, counts=None, start_deg=(0.9, 4.7), start_mm=(3.0, 8.0)):
    """A seeded synthetic sequence: n frames with random G_i that put the object about 600 mm in front of the camera, m model
    points per frame in +-50 mm, pixels with Gaussian noise (px) rounded to f32, a share of uniform outliers over the
    image, and a start Y0 = dT Y_true that is start_deg degrees and start_mm mm off.
    -> dict(p3d (n, cap, 3) f32, p2d (n, cap, 2) f32, counts (n,) i32, K (n, 9), G (n, 12), Y_true, Y0)."""
    rng = np.random.default_rng(seed)
    cap = m if cap is None else cap
    Y_true = pose(random_rot(rng), rng.uniform(-20, 20, 3))
    p3d = np.zeros((n, cap, 3), np.float32)
    p2d = np.zeros((n, cap, 2), np.float32)
    G = np.zeros((n, 12))
    for i in range(n):
        Gi = pose(random_rot(rng), np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(550, 650)]))
        G[i] = Gi[:3].reshape(12)
        p = rng.uniform(-50, 50, (m, 3)).astype(np.float32)
        c = (p.astype(np.float64) @ Y_true[:3, :3].T + Y_true[:3, 3]) @ Gi[:3, :3].T + Gi[:3, 3]
        h = c @ K_DEFAULT.T
        u = h[:, :2] / h[:, 2:3] + rng.normal(0, noise, (m, 2)) if noise > 0 else h[:, :2] / h[:, 2:3]
        bad = rng.uniform(size=m) < outliers
        u[bad] = rng.uniform([0, 0], [640, 480], (int(bad.sum()), 2))
        p3d[i, :m], p2d[i, :m] = p, u.astype(np.float32)
    v = rng.normal(size=3)
    d = rng.normal(size=3)
    dT = pose(rot(v / np.linalg.norm(v) * np.deg2rad(rng.uniform(*start_deg))), d / np.linalg.norm(d) * rng.uniform(*start_mm))
    cnt = np.full(n, m, np.int32) if counts is None else np.asarray(counts, np.int32)
    return dict(p3d=p3d, p2d=p2d, counts=cnt, K=np.tile(K_DEFAULT.reshape(1, 9), (n, 1)), G=G, Y_true=Y_true, Y0=dT @ Y_true)


def edge_cases():
    """(name, n, cap, counts, frame_w) at the row-count edges: cap and counts at every size of EDGE_SIZES, n = 1, 2 and 17
    (past kLanes = 16), ragged counts that include 0 and cap, a frame of weight 0."""
    out = []
    for s in EDGE_SIZES:
        out.append((f"n1_cap{s}", 1, s, [s], None))
    out.append(("n2_ragged", 2, 600, [257, 600], None))
    out.append(("n17_ragged", 17, 257, [0, 1, 63, 64, 65, 255, 256, 257, 0, 257, 100, 7, 200, 64, 1, 256, 129], None))
    out.append(("n17_weight0", 17, 65, [65] * 17, [1.0] * 5 + [0.0] + [1.0] * 10 + [0.5]))
    out.append(("n2_all_zero_but_one", 2, 64, [0, 64], None))
    return out


def edge_scene(n, cap, counts, seed=11):
    """scene() with m = cap real rows per frame (so that any count <= cap is backed by data) and the given counts."""
    return scene(seed, n=n, m=cap, cap=cap, counts=counts)


def record(section, payload):
    """Merge measured ratios into profiles/seq_refit_parity.json (only when ISR_RECORD_PARITY is set: tests do not write)."""
    if not os.environ.get("ISR_RECORD_PARITY"):
        return
    data = json.loads(PARITY_FILE.read_text()) if PARITY_FILE.exists() else {}
    data[section] = payload
    PARITY_FILE.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
