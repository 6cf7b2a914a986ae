"""Point-to-plane ICP with robust weights in plain NumPy f64, pass by pass: the reference of tests/test_icp_plane_cpu.py
(test infrastructure).  It restates the rule of csrc/icp_plane.hpp without its operation order: plain NumPy products, no
fma, and sums in two shapes.  Nothing here uses oracle/ or the package beyond what tests/icp_ref.py uses.

  pass it:  p = T src in f64; every source point's exact nearest target (icp_ref.search: the lowest index on equality); a pair
            counts iff d2 <= threshold^2; fitness = n / Ns, rmse = sqrt(sum d2 / n) (0 for n = 0);
            r = (p - t).n, J = [p x n, n], w(r) by the kernel; A = sum w J J^T, b = sum w J r, wr2 = sum w r^2;
            stop if  it > 0 and |d fitness| < rel_fitness and |d rmse| < rel_rmse   (status 0)
                 or  it >= max_iter                                                  (1)
                 or  n < 6                                                           (2)
                 or  A is not positive definite                                      (3),   tested in that order;
            otherwise x = solve(A, -b), T <- dT(x) T with dT's rotation that of the unit quaternion of (1, x[:3] / 2).

`shape` chooses how the reference itself rounds: "forward" sums the rows first to last and solves with np.linalg.solve,
"backward" sums them last to first and solves through a Cholesky factor.  The distance between the two trajectories is the
reference's own error E_ref: the scale to which another correct implementation may differ from it."""
import numpy as np

from .icp_ref import MARGIN, search, transform

KERNELS = ("l2", "huber", "tukey")
STATUS = ("converged", "max_iter", "n<6", "singular")


def weights(kernel, k, r):
    a = np.abs(r)
    if kernel == "l2":
        return np.ones_like(r)
    if kernel == "huber":
        return np.where(a <= k, 1.0, k / np.maximum(a, 1e-300))
    if kernel == "tukey":
        return np.where(a <= k, (1.0 - (r / k) ** 2) ** 2, 0.0)
    raise ValueError(kernel)


def step(x):
    """dT of a solution x = (alpha, beta, gamma, t)."""
    q = np.concatenate([[1.0], 0.5 * x[:3]])
    w, a, b, c = q / np.linalg.norm(q)
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                 [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                 [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]]
    T[:3, 3] = x[3:]
    return T


def _sum(rows, shape):
    if len(rows) == 0:
        return np.zeros(rows.shape[1:])
    return np.cumsum(rows if shape == "forward" else rows[::-1], axis=0)[-1]


def icp_plane_ref(src_f32, tgt_f32, nrm_f32, threshold, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
                  kernel="tukey", k=1.0, shape="forward", search_fn=search):
    """-> trajectory: a list of dicts T, fitness, rmse, n, iterations, status (None while the loop goes on), wr2, and the
    margins gap, thr_margin, ties of icp_ref.search; entry m holds the state after m updates, the last one is where the loop
    stopped.  search_fn: as in icp_ref.icp_ref (icp_ref.search_f32_lowest models a search without the f64 decision)."""
    src = np.asarray(src_f32, np.float32).astype(np.float64)
    tgt = np.asarray(tgt_f32, np.float32).astype(np.float64)
    nrm = np.asarray(nrm_f32, np.float32).astype(np.float64)
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    T[3] = [0, 0, 0, 1]
    threshold = float(threshold)
    traj, it, prev = [], 0, None
    while True:
        p = transform(T, src)
        idx, d2, gap, thr_margin, ties = search_fn(p, tgt, threshold)
        m = d2 <= threshold * threshold
        n = int(m.sum())
        fit = n / len(src)
        rmse = float(np.sqrt(_sum(d2[m], shape) / n)) if n else 0.0
        pm, tm, nm = p[m], tgt[idx[m]], nrm[idx[m]]
        r = ((pm - tm) * nm).sum(1)
        J = np.concatenate([np.cross(pm, nm), nm], 1)
        w = weights(kernel, k, r)
        A = _sum((w[:, None] * J)[:, :, None] * J[:, None, :], shape)
        b = _sum((w * r)[:, None] * J, shape)
        wr2 = float(_sum(w * r * r, shape))
        conv = it > 0 and abs(prev[0] - fit) < rel_fitness and abs(prev[1] - rmse) < rel_rmse
        status = 0 if conv else 1 if it >= max_iter else 2 if n < 6 else None
        x = None
        if status is None:
            try:
                L = np.linalg.cholesky(A)
                x = np.linalg.solve(A, -b) if shape == "forward" else np.linalg.solve(L.T, np.linalg.solve(L, -b))
                if not np.all(np.isfinite(x)):
                    status = 3
            except np.linalg.LinAlgError:
                status = 3
        traj.append(dict(T=T.copy(), fitness=fit, rmse=rmse, n=n, iterations=it, status=status, wr2=wr2, gap=gap,
                         thr_margin=thr_margin, ties=ties))
        if status is not None:
            return traj
        prev = (fit, rmse)
        T = step(x) @ T
        it += 1


def safe(traj):
    """'' if every pass of the trajectory can be compared (no tie, every decision further than MARGIN from its edge)."""
    for m, e in enumerate(traj):
        if not (e["ties"] == 0 and e["gap"] > MARGIN and e["thr_margin"] > MARGIN):
            return f"pass {m}: ties {e['ties']}, gap {e['gap']:.3e}, threshold margin {e['thr_margin']:.3e}"
    return ""


def deviation(a, b):
    """The relative distance between two states: the largest of T's (its entries against max(1, max |T|)), rmse's and sum w
    r^2's.  One figure, because a single quantity's two sums can agree to the last bit by chance (its own deviation is then 0
    and says nothing about the rounding of a third summation shape)."""
    Ta, Tb = np.asarray(a["T"], np.float64)[:3], np.asarray(b["T"], np.float64)[:3]
    rel = lambda x, y: abs(x - y) / max(abs(x), abs(y)) if x != y else 0.0
    return max(float(np.abs(Ta - Tb).max() / max(1.0, np.abs(Ta).max())), rel(a["rmse"], b["rmse"]), rel(a["wr2"], b["wr2"]))


# ------------------------------------------------------------------------------------------------ host parity
PARITY_BOUND = 16.0     # the host build may differ from the reference by this many E_ref (a third summation shape — the tree —
                        # and the compounding over three updates)
PARITY_SIZES = [(300, 700), (257, 513), (1025, 600)]


def parity_case(Ns, Nt, kernel, seed=0):
    """A random surface pair, PCA normals and a small start -> dict; k = 5 for the robust kernels (pass 0's |r| straddle it)."""
    from .icp_ref import small_pose, surface
    rng = np.random.default_rng([seed, 90, Ns, Nt])
    src, tgt = surface(rng, Ns), surface(rng, Nt)
    return dict(name=f"{kernel}_{Ns}x{Nt}", src=src, tgt=tgt, nrm=pca_normals(tgt, 16), threshold=20.0, kernel=kernel, k=5.0,
                init=small_pose(rng, 3.0, 2.0))


def parity(c, host_state, updates=3):
    """One case against a host build.  host_state(case, max_iter) -> dict T, fitness, rmse, n, iterations, status, wr2 after a
    call with that max_iter (rel_fitness = rel_rmse = 0).  Returns dict(name, unsafe, e_ref, dev, ratio, discrete): e_ref
    the largest deviation between the reference's two shapes over the trajectories of 0 .. updates updates, dev the host's
    largest deviation from the "forward" reference, discrete the first integer-valued result that differs ('' if none)."""
    e_ref = dev = 0.0
    unsafe = discrete = ""
    for m in range(updates + 1):
        kw = dict(threshold=c["threshold"], init=c["init"], max_iter=m, rel_fitness=0.0, rel_rmse=0.0, kernel=c["kernel"], k=c["k"])
        a = icp_plane_ref(c["src"], c["tgt"], c["nrm"], shape="forward", **kw)
        b = icp_plane_ref(c["src"], c["tgt"], c["nrm"], shape="backward", **kw)
        unsafe = unsafe or safe(a) or safe(b)
        h = host_state(c, m)
        e_ref = max(e_ref, deviation(a[-1], b[-1]))
        dev = max(dev, deviation(a[-1], h))
        for key in ("n", "iterations", "status", "fitness"):
            if not discrete and a[-1][key] != h[key]:
                discrete = f"max_iter {m}: {key} {h[key]} != {a[-1][key]}"
    return dict(name=c["name"], unsafe=unsafe, e_ref=e_ref, dev=dev, ratio=dev / e_ref if e_ref > 0 else float("inf") if dev else 0.0,
                discrete=discrete)


# ------------------------------------------------------------------------------------------------ clouds
def rotation_xyz(angles):
    a, b, c = angles
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def perturbed_start(rng, src, deg=3.0, trans=2.0):
    """The truth (identity) perturbed by Euler angles uniform in +-deg about the source centroid and a translation uniform
    in +-trans."""
    R = rotation_xyz(np.deg2rad(rng.uniform(-deg, deg, 3)))
    c = np.asarray(src, np.float64).mean(0)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = c - R @ c + rng.uniform(-trans, trans, 3)
    return T


def pca_normals(pts, K=16):
    """Normals by PCA over the K nearest neighbours (the point included), NumPy f64 -> f32; the sign is whatever eigh gives."""
    p = np.asarray(pts, np.float64)
    out = np.empty_like(p)
    for i0 in range(0, len(p), 512):
        q = p[i0:i0 + 512]
        d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        nb = p[np.argpartition(d2, K - 1, axis=1)[:, :K]]
        c = nb - nb.mean(1, keepdims=True)
        out[i0:i0 + 512] = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c))[1][:, :, 0]
    return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------ near ties
NEAR_TIES = {"near_tie_pos": dict(sign=1.0), "near_tie_neg": dict(sign=-1.0), "near_tie_pos_permuted": dict(sign=1.0, permute=True)}
NEAR_TIE_KERNELS = ("l2", "tukey")
NEAR_TIE_K = 2.0
NEAR_TIE_SEED = 0       # tests/test_icp_plane_cpu.py shows that this seed's normals tell the tied targets apart


def near_tie_case(name, seed=NEAR_TIE_SEED):
    """icp_ref.near_tie_case (125 sources, 216 targets, threshold 2: eight targets at one f32 distance from every source
    point) with seeded random f32 normals, so that the eight carry different normals and the winner shows in every sum."""
    from .icp_ref import near_tie_case as lattice_case
    c = lattice_case(seed=seed, **NEAR_TIES[name])
    c["nrm"] = np.random.default_rng([seed, 81]).normal(size=c["tgt"].shape).astype(np.float32)
    return c


def mean_error(T, src):
    """Mean distance between a source point's position under T and its true position (the truth is the identity)."""
    s = np.asarray(src, np.float64)
    return float(np.linalg.norm(transform(T, s) - s, axis=1).mean())
