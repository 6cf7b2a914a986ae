"""Iso-surface extraction restated in NumPy (test infrastructure): the rule of csrc/mc_extract.hpp.

Vertices are table-free: the straddling edges of each axis and their f64 interpolation come from array operations, sorted by
(owner's linear index, axis).  Triangles come from a plain Python loop over the cells through the COMMITTED table
(csrc/mc_table.hpp, read as text).  Also the volumes the CPU and GPU tests share."""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "imagesequenceregistrationfor6dposeestimationlabeling_amd" / "csrc"
TABLE = CSRC / "mc_table.hpp"


def committed_table():
    """-> (max_tris, counts (256,), rows: 256 lists of (e0, e1, e2)) as the committed header holds them."""
    text = TABLE.read_text().replace("\\\n", " ")
    width = int(re.search(r"#define ISR_MC_MAX_TRIS (\d+)", text).group(1))
    counts = [int(v) for v in re.search(r"#define ISR_MC_TRI_COUNTS(.*)", text).group(1).split(",")]
    body = re.search(r"#define ISR_MC_TRI_EDGES(.*)", text).group(1)
    rows = [[int(v) for v in r.split(",")] for r in re.findall(r"\{([^{}]*)\}", body)]
    assert len(counts) == 256 and len(rows) == 256 and all(len(r) == 3 * width for r in rows)
    tris = []
    for c, r in enumerate(rows):
        assert all(e >= 0 for e in r[:3 * counts[c]]) and all(e == -1 for e in r[3 * counts[c]:]), c
        tris.append([tuple(r[3 * t:3 * t + 3]) for t in range(counts[c])])
    return width, np.asarray(counts), tris


def edge_owner(e):
    """Cube edge e = 4 * axis + idx -> (axis, owner offset (di, dj, dk))."""
    axis, u, v = e >> 2, e & 1, e >> 1 & 1
    d = [0, 0, 0]
    o1, o2 = [a for a in range(3) if a != axis]
    d[o1], d[o2] = u, v
    return axis, tuple(d)


def case_indices(vol, iso):
    """(nx-1, ny-1, nz-1) case index of every cell: bit b set when corner (b & 1, b >> 1 & 1, b >> 2 & 1) is below."""
    below = np.asarray(vol, np.float32) < np.float32(iso)
    nx, ny, nz = below.shape
    cs = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for b in range(8):
        di, dj, dk = b & 1, b >> 1 & 1, b >> 2 & 1
        cs |= below[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk].astype(np.int64) << b
    return cs


def marching_cubes(vol, iso):
    """-> (verts (V,3) f64, tris (F,3) int32)."""
    vol = np.ascontiguousarray(vol, np.float32)
    iso = np.float32(iso)
    nx, ny, nz = vol.shape
    lin = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    below = vol < iso
    keys, pos = [], []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = below[lo] != below[hi]
        va, vb = vol[lo][cross].astype(np.float64), vol[hi][cross].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (np.float64(iso) - va) / (vb - va)
        xyz = np.stack(np.nonzero(cross), axis=1).astype(np.float64)
        xyz[:, axis] += t
        keys.append(lin[lo][cross] * 3 + axis)
        pos.append(xyz)
    keys, pos = np.concatenate(keys), np.concatenate(pos)
    order = np.argsort(keys, kind="stable")
    verts = pos[order]
    vid = np.full(nx * ny * nz * 3, -1, np.int64)
    vid[keys[order]] = np.arange(len(order))

    _, _, table = committed_table()
    cs = case_indices(vol, iso)
    tris = []
    for i, j, k in zip(*np.nonzero((cs != 0) & (cs != 255))):          # np.nonzero: C order = the cells' linear order
        for tri in table[cs[i, j, k]]:
            row = []
            for e in tri:
                axis, (di, dj, dk) = edge_owner(e)
                row.append(vid[lin[i + di, j + dj, k + dk] * 3 + axis])
            tris.append(row)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    assert (tris >= 0).all()
    return verts, tris.astype(np.int32)


# ---- volumes ----

def all_cases_volume(iso=0.3, seed=1):
    """34 x 34 x 4: the 256 corner patterns as disjoint 2 x 2 x 2 point blocks, pattern c at (1 + 2 (c % 16), 1 + 2 (c // 16), 1);
    values iso -+ U(0.1, 1), every other point below."""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.1, 1.0, (34, 34, 4))
    sign = -np.ones((34, 34, 4))
    for c in range(256):
        x, y = 1 + 2 * (c % 16), 1 + 2 * (c // 16)
        for b in range(8):
            if not c >> b & 1:
                sign[x + (b & 1), y + (b >> 1 & 1), 1 + (b >> 2 & 1)] = 1.0
    return (iso + sign * mag).astype(np.float32), iso


def random_volume(shape, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, shape).astype(np.float32)


def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def ball_field(shape, centre, radius):
    """R^2 - |x - c|^2: above inside the ball."""
    i, j, k = _grid(shape)
    return (radius ** 2 - ((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2)).astype(np.float32)


def torus_field(shape, centre, ring, tube):
    i, j, k = _grid(shape)
    rho = np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2)
    return (tube ** 2 - ((rho - ring) ** 2 + (k - centre[2]) ** 2)).astype(np.float32)


def ripple_ball(n=128):
    """A smooth field whose surface is small beside the volume: a ball of radius 0.3 n with a ripple of 3 % on it."""
    i, j, k = _grid((n, n, n))
    c = (n - 1) / 2 + 0.37
    r = np.sqrt((i - c) ** 2 + (j - c) ** 2 + (k - c) ** 2)
    return (0.3 * n - r + 0.03 * 0.3 * n * np.sin(0.2 * i) * np.sin(0.17 * j + 1.0) * np.sin(0.23 * k + 2.0)).astype(np.float32)


# ---- properties ----

def directed_edges(tris):
    t = np.asarray(tris, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def closed_and_oriented(tris):
    """Every directed triangle edge occurs exactly once and its reverse exactly once."""
    e = directed_edges(tris)
    n = int(e.max()) + 1 if len(e) else 1
    fwd, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(rev))


def euler(verts, tris):
    return len(verts) - len(directed_edges(tris)) // 2 + len(tris)


def signed_volume(verts, tris):
    p = verts[np.asarray(tris, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
