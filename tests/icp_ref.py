"""Point-to-point ICP in plain NumPy f64, pass by pass: the reference of tests/test_gpu_icp_edges.py (checked itself by
tests/test_icp_ref_cpu.py).  Nothing here uses oracle/ or the package.

The loop, as the project states it (csrc/icp_loop.hpp, PointToPoint::finish):
  pass it:  p = T src in f64; every source point's nearest target by exact brute force on doubles, the LOWEST index on
            exact equality; a pair counts iff d2 <= threshold * threshold; fitness = n / Ns, rmse = sqrt(sum d2 / n) (0 for
            n = 0);
            stop if  it > 0 and |d fitness| < rel_fitness and |d rmse| < rel_rmse   ("converged")
                 or  it >= max_iter                                                  ("max_iter")
                 or  n < 3                                                           ("n<3"),       tested in that order;
            otherwise T <- kabsch(pairs) T, it <- it + 1.
  kabsch:   sums centred before multiplying, SVD, d = sign(det) (the form of oracle/registration_oracle.py:kabsch).
A trajectory is the list of passes; entry k is the state after exactly k updates.

Beside the state every pass carries two margins, which say how far its outcome is from depending on the last bits:
  gap         smallest relative gap (d2_second - d2_best) / d2_second between the best and the second-best DISTINCT squared
              distance, over the points whose best lies within the radius (the second-best is never nearer);
  thr_margin  smallest |d - threshold| over all points;
and `ties`, the number of such points whose best distance is reached by two targets of different coordinates (targets with
the same coordinates give the same distance in any arithmetic: the lowest index wins everywhere).  A pass is safe to compare
when ties = 0, gap > MARGIN and thr_margin > MARGIN, or when its arithmetic is exact (small integer coordinates, an identity
or integer start: every d2, and its comparison with threshold^2, is exact in f32 and f64 alike) and the gap is exactly 0 or
above MARGIN: the builders below declare those passes in `exact`."""
import numpy as np

MARGIN = 1e-9


# ------------------------------------------------------------------------------------------------ the loop
def transform(T, pts):
    T = np.asarray(T, np.float64)
    return np.asarray(pts, np.float64) @ T[:3, :3].T + T[:3, 3]


def search(p, tgt, threshold):
    """Exact nearest target of every row of p (f64): (idx, d2, gap, thr_margin, ties)."""
    d2 = ((p[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)
    idx = np.argmin(d2, axis=1)                                  # first occurrence: the lowest index on equality
    best = d2[np.arange(len(p)), idx]
    near = best <= threshold * threshold * (1 + 1e-6)
    gap, ties = np.inf, 0
    if tgt.shape[0] > 1 and near.any():
        dn, bn = d2[near], best[near]
        second = np.where(dn > bn[:, None], dn, np.inf).min(1)
        fin = np.isfinite(second)
        if fin.any():
            gap = float(((second[fin] - bn[fin]) / second[fin]).min())
        same = (tgt[None, :, :] == tgt[idx[near]][:, None, :]).all(-1)
        ties = int(((dn == bn[:, None]) & ~same).any(1).sum())
    thr_margin = float(np.abs(np.sqrt(best) - threshold).min())
    return idx, best, gap, thr_margin, ties


def search_f32_lowest(p, tgt, threshold=None):
    """A model of a search WITHOUT the f64 decision of near ties: the transformed source rounded to f32, squared distances
    in f32, the lowest index on equality.  Only for showing that a case tells the two apart."""
    q = p.astype(np.float32)
    t = tgt.astype(np.float32)
    d = q[:, None, :] - t[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    idx = np.argmin(d2, axis=1)
    best = ((p - tgt[idx]) ** 2).sum(-1)
    return idx, best, np.inf, np.inf, 0


def kabsch(P, Q):
    """Rigid 4x4 T with Q ~ R P + t."""
    mp, mq = P.mean(0), Q.mean(0)
    H = (P - mp).T @ (Q - mq)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mq - R @ mp
    return T


def stiffness(P, Q):
    """(s2 + d s3) / s1 of the pairs' covariance (singular values s1 >= s2 >= s3, d = sign det): what holds the fit's
    least determined rotation axis, relative to the covariance's scale.  0: the rotation is not unique."""
    H = (P - P.mean(0)).T @ (Q - Q.mean(0))
    sv = np.linalg.svd(H)[1]
    return float((sv[1] + np.sign(np.linalg.det(H)) * sv[2]) / sv[0]) if sv[0] > 0 else 0.0


def icp_ref(src_f32, tgt_f32, threshold, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, search_fn=search):
    """-> trajectory: a list of dicts T, fitness, rmse, n, idx, iterations, stop (None while the loop goes on), gap,
    thr_margin, ties, the pairs P, Q and their stiffness; entry k holds the state after k updates, the last one is where the loop stopped."""
    src = np.asarray(src_f32, np.float32).astype(np.float64)
    tgt = np.asarray(tgt_f32, np.float32).astype(np.float64)
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
        rmse = float(np.sqrt(d2[m].sum() / n)) if n else 0.0
        conv = it > 0 and abs(prev[0] - fit) < rel_fitness and abs(prev[1] - rmse) < rel_rmse
        stop = "converged" if conv else "max_iter" if it >= max_iter else "n<3" if n < 3 else None
        P, Q = p[m], tgt[idx[m]]
        traj.append(dict(T=T.copy(), fitness=fit, rmse=rmse, n=n, idx=idx, iterations=it, stop=stop, gap=gap,
                         thr_margin=thr_margin, ties=ties, P=P, Q=Q, stiffness=None if stop else stiffness(P, Q)))
        if stop:
            return traj
        prev = (fit, rmse)
        T = kabsch(p[m], tgt[idx[m]]) @ T
        it += 1


MIN_STIFFNESS = 1e-3


def inputs_ok(traj, exact=(), degenerate=False):
    """The condition on a case's inputs: '' if every pass can be compared, else what fails.  Beside the margins, every pass
    that updates must have a unique fit (degenerate = False): the rounding of the covariance, ~1e-16 of its scale, moves the
    rotation by that over the stiffness — at MIN_STIFFNESS 1e-13 rad, far inside the 1e-9 rad the poses are compared to."""
    for k, e in enumerate(traj):
        if e["stop"] is None and not degenerate and not e["stiffness"] > MIN_STIFFNESS:
            return f"pass {k}: stiffness {e['stiffness']:.3e}: the rigid fit is not unique"
        if k in exact:
            if not (e["gap"] == 0 or e["gap"] > MARGIN):       # (exact arithmetic: d2 against threshold^2 is exact too)
                return f"exact pass {k}: gap {e['gap']:.3e}"
        elif not (e["ties"] == 0 and e["gap"] > MARGIN and e["thr_margin"] > MARGIN):
            return f"pass {k}: ties {e['ties']}, gap {e['gap']:.3e}, threshold margin {e['thr_margin']:.3e}"
    return ""


def rot_angle(Ra, Rb):
    f = np.linalg.norm(np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64))
    return float(2.0 * np.arcsin(min(1.0, f / (2.0 * np.sqrt(2.0)))))


def residual(T, P, Q):
    """Sum of squared residuals of the pairs (P, Q) under the 4x4 step T."""
    return float(((transform(T, P) - Q) ** 2).sum())


# ------------------------------------------------------------------------------------------------ clouds
def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose(R=None, t=(0, 0, 0)):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


def small_pose(rng, deg, trans):
    return pose(rotation(rng.normal(size=3), np.deg2rad(deg)), rng.uniform(-trans, trans, 3))


def surface(rng, n):
    """n points on a bumpy ellipsoid (radii 50, 35, 20 mm): a surface scan, f32."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    th, ph = np.arccos(np.clip(d[:, 2], -1, 1)), np.arctan2(d[:, 1], d[:, 0])
    return (d * [50.0, 35.0, 20.0] * (1 + 0.12 * np.sin(3 * th) * np.cos(2 * ph))[:, None]).astype(np.float32)


def blob(rng, n, sigma=(30.0, 20.0, 10.0)):
    return (rng.normal(size=(n, 3)) * sigma).astype(np.float32)


def case(name, src, tgt, threshold, init=None, exact=(), kmax=None, **kw):
    """exact: the passes whose arithmetic is exact; kmax: compare k = 0 .. kmax only (None: to the end of the loop)."""
    c = dict(name=name, src=np.ascontiguousarray(src, np.float32), tgt=np.ascontiguousarray(tgt, np.float32),
             threshold=float(threshold), init=np.eye(4) if init is None else np.asarray(init, np.float64),
             exact=tuple(exact), kmax=kmax, rel=(1e-6, 1e-6), degenerate=False)
    c.update(kw)
    return c


def trajectory(c, max_iter=12):
    return icp_ref(c["src"], c["tgt"], c["threshold"], c["init"], max_iter, *c["rel"])


# (a) sizes -----------------------------------------------------------------------------------------------
# one 256-target tile against two key ranges (256 | 257), a last range of ONE target (257, 513, 1025), one query per lane
# against four (1023 | 1024), ragged last workgroups and waves (63, 65, 255, 257, 1025, 1281), rows in Morton order
# (min(Ns, Nt) > 256) and as given.  Nt = 1 and 2 go with Ns <= 2 only: three or more points matched to one or two targets
# have no unique rigid fit (those are the S = 0 and collinear cases of (e)).
SIZE_PAIRS = [(1, 1), (2, 1), (1, 257), (2, 2), (2, 1025), (3, 3), (4, 3), (63, 255), (64, 256), (65, 257), (255, 513),
              (256, 257), (257, 256), (257, 513), (257, 1025), (1023, 255), (1023, 513), (1024, 257), (1024, 1025),
              (1025, 3), (1025, 1025), (1281, 513), (1281, 1025)]


def size_case(Ns, Nt, seed=0):
    rng = np.random.default_rng([seed, Ns, Nt])
    src, tgt = surface(rng, Ns), surface(rng, Nt)
    if min(Ns, Nt) < 10:          # a handful of points: each source point beside a target of its own (row i beside target i mod
        src = (tgt[np.arange(Ns) % Nt] + rng.normal(size=(Ns, 3))).astype(np.float32)    # Nt), or the pairs have no unique fit
    return case(f"size_{Ns}x{Nt}", src, tgt, 200.0 if min(Ns, Nt) < 10 else 20.0, small_pose(rng, 3.0, 2.0))


def count_case(n0, seed=0):
    """A threshold that leaves pass 0 exactly n0 correspondences (halfway between two neighbour distances)."""
    rng = np.random.default_rng([seed, 77, n0])
    src, tgt = surface(rng, 65), surface(rng, 300)
    init = small_pose(rng, 2.0, 1.0)
    d = np.sort(np.sqrt(search(transform(init, src.astype(np.float64)), tgt.astype(np.float64), 1e9)[1]))
    thr = 0.5 * d[0] if n0 == 0 else 0.5 * (d[n0 - 1] + d[n0])
    return case(f"count_{n0}", src, tgt, thr, init, n0=n0)


def origin_case(seed=0):
    """One source point and one target, both the origin, T = I: fitness 1, rmse 0, one correspondence."""
    return case("origin_1x1", np.zeros((1, 3)), np.zeros((1, 3)), 1.0, exact=(0,))


# (b) the stopping rule -----------------------------------------------------------------------------------
def same_cloud_case(seed=0):
    rng = np.random.default_rng([seed, 78])
    c = surface(rng, 300)
    return case("source_is_target", c, c, 5.0)


def never_converges_case(seed=0):
    c = size_case(257, 513, seed)
    c.update(name="rel_zero", rel=(0.0, 0.0))
    return c


def boundary_case(inside, seed=0):
    """Integer coordinates, every source point exactly 5 from its target (offset (3, 4, 0)), the others 15 or more away:
    threshold 5.0 counts every pair (25 <= 25), the next double below counts none."""
    rng = np.random.default_rng([seed, 79])
    cells = rng.permutation(8 ** 3)[:100]
    tgt = 20.0 * np.stack([cells // 64, (cells // 8) % 8, cells % 8], 1)
    thr = 5.0 if inside else float(np.nextafter(5.0, 0.0))
    return case("radius_5_in" if inside else "radius_5_out", tgt - [3.0, 4.0, 0.0], tgt, thr, exact=(0,))


# (c) ties ------------------------------------------------------------------------------------------------
def lattice():
    g = np.arange(0.0, 11.0, 2.0)
    tgt = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)             # x-major, 216 rows
    h = np.arange(1.0, 10.0, 2.0)
    src = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)             # the 125 cell centres
    return src, tgt


def near_tie_case(sign=1.0, permute=False, seed=0):
    """Every source point has eight targets at the same f32 distance; in f64 the (+,+,+) corner (sign = 1; the (-,-,-)
    corner for sign = -1) is nearer by a relative 1.3e-9.  One update moves the cloud by sign * (1, 1, 1); the lowest-index
    winner of an f32 search moves it by (-1, -1, -1)."""
    src, tgt = lattice()
    if permute:
        src = src[np.random.default_rng([seed, 80]).permutation(len(src))]
    name = "near_tie_" + ("pos" if sign > 0 else "neg") + ("_permuted" if permute else "")
    return case(name, src, tgt, 2.0, pose(t=sign * np.array([1e-9, 2e-9, 3e-9])), step=sign * np.ones(3))


def exact_tie_case(seed=0):
    """The lattice at the identity: pass 0 is exact arithmetic, the lowest index of the eight wins.  Compared for k = 0, 1."""
    src, tgt = lattice()
    return case("exact_tie", src, tgt, 2.0, exact=(0,), kmax=1, step=-np.ones(3))


def duplicate_case(Ns, seed=0):
    """A 700-row target and, in `tgt2`, the same target twice: every source point has two targets at the same distance
    (the same coordinates, 700 rows apart) in every pass."""
    rng = np.random.default_rng([seed, 81, Ns])
    src, tgt = surface(rng, Ns), surface(rng, 700)
    return case(f"duplicates_{Ns}", src, tgt, 20.0, small_pose(rng, 3.0, 2.0), tgt2=np.concatenate([tgt, tgt]))


# (d) the tile cull ---------------------------------------------------------------------------------------
def cull_case(kind, seed=0):
    rng = np.random.default_rng([seed, 82])
    src, tgt = surface(rng, 1025), surface(rng, 1025)
    init, thr = small_pose(rng, 2.0, 1.0), 8.0
    if kind == "sorted_x":                          # tight, disjoint tile boxes
        tgt, src = tgt[np.argsort(tgt[:, 0], kind="stable")], src[np.argsort(src[:, 0], kind="stable")]
    elif kind == "far_rows":
        # the first 256 source rows beyond the radius.  With one query per lane (the plan below 1024 rows, hence 1023 of them)
        # they are workgroup 0 of the search: from the second pass on the cull lets it leave without posting, their slots stay
        # empty, and the pass after that starts those lanes without a warm neighbour.  With four queries per lane (the plan
        # knob) they are one wave of a workgroup whose other waves post.
        src = src[np.argsort(src[:, 0], kind="stable")][:1023]
        src[:256] += np.float32(500.0)
    elif kind == "shuffled":                        # every wave's box is the whole cloud
        src = src[rng.permutation(len(src))]
    elif kind == "small_threshold":
        thr = 1.5
    else:
        raise ValueError(kind)
    return case(f"cull_{kind}", src, tgt, thr, init, spatial_order=(kind == "small_threshold"))


CULL_KINDS = ["sorted_x", "far_rows", "shuffled", "small_threshold"]


# (e) geometry of the update: one step, a large threshold, unambiguous pass-0 neighbours -------------------
def _moved(rng, tgt, deg, trans, noise=0.0):
    """A source that the inverse of a small motion takes off the target (pairs i <-> i), optionally with noise."""
    M = small_pose(rng, deg, trans)
    src = transform(np.linalg.inv(M), tgt.astype(np.float64))
    return src + noise * rng.normal(size=src.shape)


def geometry_case(kind, seed=0):
    rng = np.random.default_rng([seed, 83])
    if kind == "coplanar":                          # both clouds in the plane z = 7
        tgt = np.concatenate([rng.uniform(-40, 40, (60, 2)), np.full((60, 1), 7.0)], 1).astype(np.float32)
        src = transform(pose(rotation([0, 0, 1], 0.03), [0.4, -0.3, 0.0]), tgt - [0, 0, 7.0]) + [0, 0, 7.0]
        src[:, :2] += 0.2 * rng.normal(size=(60, 2))
    elif kind == "reflection":                      # a thin slab against its mirror image: Kabsch's d = -1 branch
        tgt = blob(rng, 80, (30.0, 20.0, 1.0))
        src = transform(pose(rotation(rng.normal(size=3), 0.02)), tgt * [1.0, 1.0, -1.0])
    elif kind == "three_pairs":
        tgt = np.array([[10.0, 0, 0], [-20.0, 15, 3], [4.0, -30, 11]], np.float32)
        src = _moved(rng, tgt, 4.0, 2.0, 0.3)
    elif kind == "volume":                          # a well-conditioned 3-D set: the case the offsets of (f) shift
        tgt = blob(rng, 300)
        src = _moved(rng, tgt, 3.0, 1.0, 0.3)
    else:
        raise ValueError(kind)
    return case(f"geometry_{kind}", src, tgt, 100.0, kmax=1)


GEOMETRY_KINDS = ["coplanar", "reflection", "three_pairs"]


def collinear_case(seed=0):
    """Integers times (1.5, -1, 0.5), and on the same line the source: the targets' multipliers plus eighths that no rigid
    motion takes out (the optimum's residual is not 0), moved by an offset.  Every sum is exact; no unique rotation."""
    v = np.array([1.5, -1.0, 0.5])
    k = np.array([-8.0, -4.0, 0.0, 3.0, 7.0, 12.0])
    m = k + [0.25, -0.25, 0.5, 0.0, -0.5, 0.25]
    return case("collinear", m[:, None] * v + [0.5, 0.25, -0.75], k[:, None] * v, 100.0, kmax=1, exact=(0,), degenerate=True)


def one_target_case(seed=0):
    """Every source point matched to the one target: S = 0 — exactly, on 32 points with small integer coordinates (every sum,
    the means included, is exact in f64), so that the fit is the identity rotation and not the rounding's."""
    rng = np.random.default_rng([seed, 84])
    return case("one_target", rng.integers(-8, 9, (32, 3)), [[3.0, -2.0, 1.0]], 100.0, kmax=1, exact=(0,), degenerate=True)


# (f) distance from the origin ----------------------------------------------------------------------------
OFFSETS = [700.0, 3000.0, 10000.0]


def offset_case(offset, seed=0):
    c = geometry_case("volume", seed)
    # the same f32 clouds, shifted in f64 and rounded: the one-step neighbours stay pairs i <-> i
    c.update(name=f"offset_{int(offset)}", src=(c["src"].astype(np.float64) + offset).astype(np.float32),
             tgt=(c["tgt"].astype(np.float64) + offset).astype(np.float32), kmax=1, offset=offset)
    return c


def offset_lockstep_case(seed=0):
    c = size_case(257, 513, seed)
    c.update(name="offset_700_lockstep", src=(c["src"].astype(np.float64) + 700.0).astype(np.float32),
             tgt=(c["tgt"].astype(np.float64) + 700.0).astype(np.float32))
    R = c["init"][:3, :3]
    c["init"] = pose(R, c["init"][:3, 3] + 700.0 - R @ np.full(3, 700.0))      # the same motion about the shifted cloud
    return c


def all_cases(seed=0):
    """Every case the GPU module runs, by name."""
    cs = [size_case(a, b, seed) for a, b in SIZE_PAIRS] + [count_case(n, seed) for n in range(4)]
    cs += [origin_case(seed), same_cloud_case(seed), never_converges_case(seed), boundary_case(True, seed),
           boundary_case(False, seed), near_tie_case(1.0, False, seed), near_tie_case(-1.0, False, seed),
           near_tie_case(1.0, True, seed), exact_tie_case(seed), duplicate_case(255, seed), duplicate_case(257, seed)]
    cs += [cull_case(k, seed) for k in CULL_KINDS] + [geometry_case(k, seed) for k in GEOMETRY_KINDS + ["volume"]]
    cs += [collinear_case(seed), one_target_case(seed)] + [offset_case(o, seed) for o in OFFSETS] + [offset_lockstep_case(seed)]
    return {c["name"]: c for c in cs}


SEED = 0            # the seed of every case the GPU module runs; tests/test_icp_ref_cpu.py checks the input conditions for it
_CASES, _TRAJ = {}, {}


def cases(seed=SEED):
    if seed not in _CASES:
        _CASES[seed] = all_cases(seed)
    return _CASES[seed]


def reference(name, seed=SEED):
    """The case's trajectory (max_iter = 12), computed once and shared: do not modify it."""
    if (name, seed) not in _TRAJ:
        _TRAJ[name, seed] = trajectory(cases(seed)[name])
    return _TRAJ[name, seed]
