"""CPU: iso-surface extraction as host code (csrc/mc_extract.hpp through isr_mc_count_host / isr_mc_emit_host): the committed
case table against its generator and the rule it states, the output against the NumPy restatement of tests/mc_ref.py bit for
bit, exact geometry on a plane, topology and orientation on balls and a torus, the edge cases, argument errors without a
device, and the ctypes table against include/isr_mc.h."""
import ctypes
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
from tests import density_ref, mc_ref

ROOT = Path(__file__).resolve().parent.parent
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_mc_table", ROOT / "tools" / "gen_mc_table.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same(got, want):
    (gv, gt), (wv, wt) = got, want
    assert gv.dtype == np.float64 and gt.dtype == np.int32 and gv.shape == wv.shape and gt.shape == wt.shape
    assert gv.shape[1:] == (3,) and gt.shape[1:] == (3,)
    assert np.array_equal(gv.view(np.uint64), wv.view(np.uint64)) and np.array_equal(gt, wt)


# ---- the table ----

def test_committed_table_is_the_generators(gen):
    assert mc_ref.TABLE.read_text() == gen.render()


def test_table_follows_the_rule_for_all_256_cases(gen):
    width, counts, table = mc_ref.committed_table()
    assert width == counts.max() == max(len(t) for t in table)
    # the kernel and the table width take the generator's figure
    assert "kMaxTris = ISR_MC_MAX_TRIS" in (mc_ref.CSRC / "mc_extract.hpp").read_text()
    for case in range(256):
        tris = table[case]
        below = [bool(case >> b & 1) for b in range(8)]
        crossing = {e for e, (a, b) in enumerate(gen.EDGES) if below[a] != below[b]}
        assert {e for t in tris for e in t} == crossing, case                   # every crossing edge is used
        directed = [(t[n], t[(n + 1) % 3]) for t in tris for n in range(3)]
        assert len(set(directed)) == len(directed), case
        rim = [(a, b) for a, b in directed if (b, a) not in directed]           # the loops: what no other triangle closes
        assert sorted(a for a, _ in rim) == sorted(b for _, b in rim) == sorted(crossing), case     # closed: one in, one out
        # the face rule, restated: per face, from its four flags
        want = set()
        for axis in range(3):
            for side in range(2):
                corners = [b for b in range(8) if (b >> axis & 1) == side]
                edges = [e for e, (a, b) in enumerate(gen.EDGES) if a in corners and b in corners and below[a] != below[b]]
                if len(edges) == 2:
                    want.add(frozenset(edges))
                elif len(edges) == 4:
                    for c in corners:
                        if below[c]:
                            want.add(frozenset(e for e in edges if c in gen.EDGES[e]))
                else:
                    assert not edges
        assert {frozenset(s) for s in rim} == want and len(rim) == len(want), case
        # a chord (a triangle edge that is no face segment) never lies in a face of the cube: the neighbouring cell cannot draw it too
        on_a_face = lambda a, b: any(len({gen.CORNERS[c][ax] for e in (a, b) for c in gen.EDGES[e]}) == 1 for ax in range(3))
        assert all(on_a_face(a, b) for a, b in rim), case
        assert not any(on_a_face(a, b) for a, b in directed if (b, a) in directed), case
        # loops in the order of their lowest edge; each a fan from its lowest edge that allows a fan without such a chord
        fans = {}
        for t in tris:
            fans.setdefault(t[0], []).append(t)
        loops = [[apex, fan[0][1]] + [t[2] for t in fan] for apex, fan in fans.items()]
        assert sorted(e for lp in loops for e in lp) == sorted(crossing), case
        assert [min(lp) for lp in loops] == sorted(min(lp) for lp in loops), case
        for lp in loops:
            assert all(t == (lp[0], lp[n], lp[n + 1]) for n, t in enumerate(fans[lp[0]], start=1)), case
            for e in sorted(lp):
                r = lp[lp.index(e):] + lp[:lp.index(e)]
                if not any(on_a_face(r[0], r[n]) for n in range(2, len(r) - 1)):
                    break
            assert e == lp[0], case


# ---- against the NumPy restatement ----

@pytest.fixture(scope="module")
def all_cases():
    vol, iso = mc_ref.all_cases_volume()
    return vol, iso, mc_ref.marching_cubes(vol, iso)


def test_all_cases_volume(hip_lib, all_cases):
    vol, iso, want = all_cases
    assert vol.shape == (34, 34, 4)
    assert set(np.unique(mc_ref.case_indices(vol, iso)).tolist()) == set(range(256))
    got = ops.marching_cubes_host(vol, iso)
    assert mc_ref.closed_and_oriented(got[1])
    _same(got, want)


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 2, 2), (9, 9, 9), (17, 13, 9)])
def test_random_volumes_equal_the_restatement(hip_lib, shape):
    vol = mc_ref.random_volume(shape, seed=sum(shape))
    got = ops.marching_cubes_host(vol, 0.5)
    assert len(got[0]) > 0
    _same(got, mc_ref.marching_cubes(vol, 0.5))


def test_plane_is_exact(hip_lib):
    """v = i + 2 j + 3 k is exact in f32 and so are iso - va and vb - va: one f64 division at magnitudes below 1e2."""
    i, j, k = np.meshgrid(np.arange(12), np.arange(10), np.arange(8), indexing="ij")
    vol = (i + 2 * j + 3 * k).astype(np.float32)
    verts, tris = ops.marching_cubes_host(vol, 20.5)
    assert len(verts) > 100 and len(tris) > 100
    err = np.abs(verts @ np.array([1.0, 2.0, 3.0]) - 20.5)
    print("plane: worst |n.x - iso| =", err.max())
    assert err.max() <= 1e-12
    _same((verts, tris), mc_ref.marching_cubes(vol, 20.5))


# ---- topology and orientation ----

C1, C2 = (11.3, 12.1, 11.7), (6.2, 6.4, 6.1)


def test_one_ball(hip_lib):
    vol = mc_ref.ball_field((24, 24, 24), C1, 8.0)
    assert (vol[0] < 0).all() and (vol[-1] < 0).all() and (vol[:, 0] < 0).all() and (vol[:, :, -1] < 0).all()
    verts, tris = ops.marching_cubes_host(vol, 0.0)
    assert mc_ref.closed_and_oriented(tris) and mc_ref.euler(verts, tris) == 2
    p = verts[tris.astype(np.int64)]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", normal, p.mean(axis=1) - np.asarray(C1)) > 0).all()      # outward: towards the below side
    assert mc_ref.signed_volume(verts, tris) > 0


def test_two_balls_and_a_torus(hip_lib):
    two = np.maximum(mc_ref.ball_field((24, 24, 24), C2, 4.0), mc_ref.ball_field((24, 24, 24), (16.6, 15.9, 16.3), 5.0))
    verts, tris = ops.marching_cubes_host(two, 0.0)
    assert mc_ref.closed_and_oriented(tris) and mc_ref.euler(verts, tris) == 4 and mc_ref.signed_volume(verts, tris) > 0
    torus = mc_ref.torus_field((24, 24, 24), C1, 7.0, 2.6)
    verts, tris = ops.marching_cubes_host(torus, 0.0)
    assert mc_ref.closed_and_oriented(tris) and mc_ref.euler(verts, tris) == 0 and mc_ref.signed_volume(verts, tris) > 0


# ---- edge cases ----

def test_empty_surfaces(hip_lib):
    vol = mc_ref.random_volume((5, 4, 3), 2)
    for iso in (2.0, -1.0):                     # all below, all above
        verts, tris = ops.marching_cubes_host(vol, iso)
        assert verts.shape == (0, 3) and tris.shape == (0, 3) and verts.dtype == np.float64 and tris.dtype == np.int32


def test_a_corner_equal_to_iso_is_above(hip_lib):
    """One point at iso among points below: its three owned edges start AT it (parameter exactly 0), the three edges that end
    at it reach it (exactly 1): six vertices at one position with six ids, eight triangles."""
    vol = np.full((3, 3, 3), -1.0, np.float32)
    vol[1, 1, 1] = 0.25
    verts, tris = ops.marching_cubes_host(vol, 0.25)
    assert verts.shape == (6, 3) and np.array_equal(verts, np.ones((6, 3))) and tris.shape == (8, 3)
    assert sorted(np.unique(tris).tolist()) == list(range(6)) and all(len(set(t)) == 3 for t in tris.tolist())
    assert mc_ref.closed_and_oriented(tris) and mc_ref.euler(verts, tris) == 2
    _same((verts, tris), mc_ref.marching_cubes(vol, 0.25))


def test_check_finite(hip_lib):
    vol = mc_ref.random_volume((4, 5, 6), 3)
    vol[2, 3, 1] = np.nan
    with pytest.raises(ValueError):
        ops.marching_cubes_host(vol, 0.5)
    # the switch: a NaN counts as above, counting and emitting agree, and the restatement says the same
    got = ops.marching_cubes_host(vol, 0.5, check_finite=False)
    want = mc_ref.marching_cubes(vol, 0.5)
    assert np.isnan(got[0]).any()
    _same(got, want)


def test_argument_errors_without_a_device(hip_lib):
    L = hip_lib
    vol = mc_ref.random_volume((4, 3, 2), 4)
    counts = np.zeros(2, np.int32)
    assert L.isr_mc_count_host(vp(vol), 4, 3, 2, 0.5, vp(counts)) == 0
    V, F = int(counts[0]), int(counts[1])
    assert V > 0 and F > 0
    verts, tris = np.zeros((V, 3)), np.zeros((F, 3), np.int32)
    nb = L.isr_mc_workspace_bytes(4, 3, 2)
    assert nb > 0
    ws = np.zeros(nb, np.uint8)

    def refused(nx, ny, nz, vol_p=vp(vol), iso=0.5):
        """By all four entries, the device ones before any device access."""
        for rc in (L.isr_mc_count(vol_p, nx, ny, nz, iso, vp(counts), vp(ws), nb, None),
                   L.isr_mc_emit(vol_p, nx, ny, nz, iso, vp(ws), nb, vp(verts), V, vp(tris), F, None),
                   L.isr_mc_count_host(vol_p, nx, ny, nz, iso, vp(counts)),
                   L.isr_mc_emit_host(vol_p, nx, ny, nz, iso, vp(verts), V, vp(tris), F)):
            assert rc == -1 and L.isr_last_error()

    refused(4, 3, 2, vol_p=None)
    refused(1, 3, 2)
    refused(4, 1, 2)
    refused(4, 3, 1)
    refused(4, 3, 1025)
    refused(1024, 1024, 257)                                     # above 2^28 points: refused before vol is read
    assert b"2^28" in L.isr_last_error()
    refused(4, 3, 2, iso=float("nan"))
    assert L.isr_mc_workspace_bytes(1, 3, 2) == 0 and L.isr_mc_workspace_bytes(1024, 1024, 257) == 0 and L.isr_last_error()
    assert L.isr_mc_workspace_bytes(1024, 1024, 256) > 0
    # null outputs and workspaces, a short workspace
    assert L.isr_mc_count(vp(vol), 4, 3, 2, 0.5, None, vp(ws), nb, None) == -1
    assert L.isr_mc_count(vp(vol), 4, 3, 2, 0.5, vp(counts), None, nb, None) == -1
    assert L.isr_mc_count(vp(vol), 4, 3, 2, 0.5, vp(counts), vp(ws), nb - 1, None) == -1
    assert b"workspace" in L.isr_last_error()
    assert L.isr_mc_emit(vp(vol), 4, 3, 2, 0.5, vp(ws), nb - 1, vp(verts), V, vp(tris), F, None) == -1
    assert b"workspace" in L.isr_last_error()
    assert L.isr_mc_emit(vp(vol), 4, 3, 2, 0.5, None, nb, vp(verts), V, vp(tris), F, None) == -1
    assert L.isr_mc_emit(vp(vol), 4, 3, 2, 0.5, vp(ws), nb, None, V, vp(tris), F, None) == -1
    assert L.isr_mc_emit(vp(vol), 4, 3, 2, 0.5, vp(ws), nb, vp(verts), V, None, F, None) == -1
    assert L.isr_mc_emit(vp(vol), 4, 3, 2, 0.5, vp(ws), nb, vp(verts), -1, vp(tris), F, None) == -1
    assert L.isr_mc_count_host(vp(vol), 4, 3, 2, 0.5, None) == -1
    assert L.isr_mc_emit_host(vp(vol), 4, 3, 2, 0.5, None, V, vp(tris), F) == -1
    # short V or F
    assert L.isr_mc_emit_host(vp(vol), 4, 3, 2, 0.5, vp(verts), V - 1, vp(tris), F) == -1
    assert L.isr_mc_emit_host(vp(vol), 4, 3, 2, 0.5, vp(verts), V, vp(tris), F - 1) == -1
    assert b"the volume gives" in L.isr_last_error()
    # longer ones: every element written, rows past the totals 0 and -1
    lv, lt = np.full((V + 3, 3), np.nan), np.full((F + 2, 3), 7, np.int32)
    assert L.isr_mc_emit_host(vp(vol), 4, 3, 2, 0.5, vp(lv), V + 3, vp(lt), F + 2) == 0
    want = ops.marching_cubes_host(vol, 0.5)
    _same((lv[:V], lt[:F]), want)
    assert (lv[V:] == 0).all() and (lt[F:] == -1).all()
    with pytest.raises(_capi.IsrError):
        import torch
        ops.marching_cubes(torch.zeros(4, 4, 4), 0.5)              # a CPU tensor: there is no CPU fallback


def test_mc_signatures_match_the_header(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_mc.h").read_text(), flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(isr_mc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(decls) == sorted(_capi.MC_SIGNATURES) == sorted(
        ["isr_mc_workspace_bytes", "isr_mc_count", "isr_mc_emit", "isr_mc_count_host", "isr_mc_emit_host"])
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_mc.h but not exported"
        assert len(_capi.MC_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    others = (_capi.SIGNATURES, _capi.FIELD_SIGNATURES, _capi.FPS_SIGNATURES, _capi.DENSITY_SIGNATURES)
    assert not any(set(_capi.MC_SIGNATURES) & set(o) for o in others)
    for other in ("isr_hip.h", "isr_field.h", "isr_fps.h", "isr_density.h"):
        assert "isr_mc_" not in re.sub(r"/\*.*?\*/", "", (ROOT / "include" / other).read_text(), flags=re.S)


# ---- the reference-named entry's coordinates ----

def test_forPC_coordinate_maps_on_an_8_cubed_grid(hip_lib):
    H = 4
    Ws, bs = density_ref.fixture(H, 16, 2, seed=3)
    field = DensityField(Ws, bs, density_ref.frequencies(H), 10.0, None)
    t = np.linspace(-1, 1, 8).astype(np.float32)
    grid = field.grid_densities_host(8)
    assert grid.shape == (8, 8, 8) and grid[1, 2, 3] == field.eval_host(np.array([[t[1], t[2], t[3]]], np.float32))[0]
    thr = float(np.median(grid))
    verts, tris = ops.marching_cubes_host(grid, thr)
    assert len(verts) > 10 and verts.min() >= 0 and verts.max() <= 7
    assert np.array_equal(DensityField._pc_coords(verts, 8, "index"), verts)
    assert np.array_equal(DensityField._pc_coords(verts, 8, "reference"), (verts - 4) / 4)      # nerf.py:701 at res 8
    assert np.array_equal(DensityField._pc_coords(verts, 128, "reference"), (verts - 64) / 64)
    g = DensityField._pc_coords(verts, 8, "grid")
    assert np.array_equal(g, -1 + 2 * verts / 7)
    # "grid" is where the densities were evaluated: integer coordinates land on the linspace; "reference" is not
    whole = verts == np.round(verts)
    assert np.abs(g[whole] - np.linspace(-1, 1, 8)[verts[whole].astype(int)]).max() < 1e-15
    corners = np.array([[0.0, 0, 0], [7.0, 7, 7]])
    assert np.array_equal(DensityField._pc_coords(corners, 8, "grid"), [[-1, -1, -1], [1, 1, 1]])
    assert np.array_equal(DensityField._pc_coords(corners, 8, "reference"), [[-1, -1, -1], [0.75, 0.75, 0.75]])
    with pytest.raises(ValueError):
        field.batched_forward_forPC(coords="world")
    with pytest.raises(_capi.IsrError):
        field.batched_forward_forPC(res=8)                       # built without a device: there is no CPU fallback
