"""Shared by the farthest-point-sampling tests (not a test module): the rule of csrc/fps.hpp as a plain NumPy f32 loop, the
f64 invariant every valid f32 sequence satisfies, and the clouds the tests use."""
import numpy as np

# Each of dx, dy, dz carries one rounding (u = 2^-24 relative), the square and the two fused adds at most four more on d:
# <= 8 u relative error on a squared distance, doubled for the two values an arg-max compares.
INVARIANT_SLACK = 16 * 2.0 ** -24


def fps_numpy(pts, K, start=0):
    """pts (len,3) -> (idx (K,) int32, radius2 (K,) f32): s_0 = start, mind = +inf, and per step
    d = fmaf(dz,dz, fmaf(dy,dy, dx*dx)) in f32, mind = fminf(mind, d), the largest mind wins, the lowest index on ties
    (np.argmax returns the first maximum).  An fmaf is the f64 product (exact for f32 factors) plus the addend, rounded to
    f32 once: exact on integer lattices, which is where the tests compare this loop index by index."""
    p = np.ascontiguousarray(pts, np.float32)
    n = len(p)
    idx = np.full(K, -1, np.int32)
    rad = np.zeros(K, np.float32)
    mind = np.full(n, np.inf, np.float32)
    s, r = int(start), np.float32(np.inf)
    for k in range(min(K, n)):
        idx[k], rad[k] = s, r
        d = (p - p[s]).astype(np.float32)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        t = (dx * dx).astype(np.float32)
        t = (dy.astype(np.float64) * dy.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
        t = (dz.astype(np.float64) * dz.astype(np.float64) + t.astype(np.float64)).astype(np.float32)
        mind = np.minimum(mind, t)
        s = int(np.argmax(mind))
        r = mind[s]
    return idx, rad


def invariant_deficit(pts, idx):
    """Replay the sequence in f64: at every step the selected point's f64 min-distance^2 over the f64 maximum over all points.
    -> the smallest such ratio (1.0: every selection was an exact f64 arg-max)."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    mind = np.full(len(p), np.inf)
    worst = 1.0
    for k in range(1, len(idx)):
        mind = np.minimum(mind, ((p - p[idx[k - 1]]) ** 2).sum(1))
        top = mind.max()
        if top > 0:
            worst = min(worst, mind[idx[k]] / top)
    return worst


def lattice(nx, ny, nz, seed):
    """The integer lattice nx x ny x nz in shuffled order: every distance is exact in f32 and ties are everywhere."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(np.random.default_rng(seed).permutation(g).astype(np.float32))


def duplicates(reps):
    """3 distinct points, the triple repeated `reps` times."""
    return np.tile(np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32), (reps, 1))
