"""Shared by the ADD-S bound tests (not a test module): the sum the brackets of isr_adds_bounds must enclose, as plain f64
brute force — no KD-tree, no kernel of this project — and the geometry of a DistField restated in f64.

    adds_sums   per item   sum_v min_s |Tq v - Tt s|   with Tt APPLIED AS GIVEN (rigid or not, None = identity)
    half_widths per item and vertex   r_v = |x - centre(cell that holds x)|,  x = Tt^-1 Tq v  for a rigid Tt
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_WORK = 1 << 16      # elements of the (vertices x cloud) distance block: two f64 blocks of this size stay in the cache


def _T(T, B=None):
    """(B,12) / (B,3,4) / None -> (B,3,4) f64."""
    if T is None:
        return np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), (B, 1, 1))
    return np.asarray(T, np.float64).reshape(-1, 3, 4)


def _min_dist_sum(q, t):
    """sum over the rows of q (V,3) of the distance to the nearest row of t (S,3): coordinate differences, no expansion of
    the square (nothing cancels), squared distances minimised and one sqrt per vertex."""
    rows = max(1, _WORK // len(t))
    tx, ty, tz = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1]), np.ascontiguousarray(t[:, 2])
    total = 0.0
    for v0 in range(0, len(q), rows):
        c = q[v0:v0 + rows]
        d2 = np.subtract.outer(c[:, 0], tx)
        d2 *= d2
        for a, ta in ((1, ty), (2, tz)):
            w = np.subtract.outer(c[:, a], ta)
            w *= w
            d2 += w
        total += float(np.sqrt(d2.min(axis=1)).sum())
    return total


def adds_sums(verts, cloud, Tq, Tt=None, workers=8):
    """verts (V,3) f32, cloud (S,3) f32, Tq / Tt (B,12) or (B,3,4) -> (B,) f64: V x ADD-S of every item (inference.py:118-120
    with the mean left as a sum).  Both clouds are moved in f64; the items are independent and spread over threads."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    s = np.asarray(cloud, np.float32).astype(np.float64)
    Tq = _T(Tq)
    Tt = _T(Tt, len(Tq))
    assert Tq.shape == Tt.shape, (Tq.shape, Tt.shape)

    def item(b):
        return _min_dist_sum(v @ Tq[b, :, :3].T + Tq[b, :, 3], s @ Tt[b, :, :3].T + Tt[b, :, 3])

    if len(Tq) < 4 or workers <= 1:
        return np.array([item(b) for b in range(len(Tq))])
    with ThreadPoolExecutor(workers) as ex:
        return np.array(list(ex.map(item, range(len(Tq)))))


def cell_centres(fld, cells):
    """f64 centres of the cells (…,3) int (ix, iy, iz) of a DistField."""
    return np.asarray(fld.grid_min, np.float64) + float(fld.h) * (np.asarray(cells, np.float64) + 0.5)


def half_widths(verts, Tq, Tt, fld):
    """-> (r (B,V) f64, inside (B,V) bool).  x = Tt^-1 Tq v in f64 with Tt inverted as the rigid motion it must be here
    (R^T, -R^T t); the cell is floor((x - grid_min) / h) clamped to the grid — the nearest cell for a point outside — and
    r = |x - centre|.  On a face, edge or corner the neighbouring cells give the same r.  inside: grid_min <= x < far corner."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    Tq = _T(Tq)
    Tt = _T(Tt, len(Tq))
    R = np.einsum("bki,bkj->bij", Tt[:, :, :3], Tq[:, :, :3])
    t = np.einsum("bki,bk->bi", Tt[:, :, :3], Tq[:, :, 3] - Tt[:, :, 3])
    x = np.einsum("bij,vj->bvi", R, v) + t[:, None, :]
    f = (x - np.asarray(fld.grid_min, np.float64)) / float(fld.h)
    dims = np.asarray(fld.dims, np.float64)
    cell = np.clip(np.floor(f), 0.0, dims - 1.0)
    r = np.linalg.norm(x - cell_centres(fld, cell), axis=-1)
    return r, ((f >= 0.0) & (f < dims)).all(axis=-1)
