"""CPU: isr_knn_host and isr_local_frames_host (csrc/knn.hpp compiled for the host) against NumPy restatements
(tests/knn_ref.py): the neighbour rows as integers and bits against a brute-force (d2, index) sort, the frames against
numpy.linalg.eigh within 100 x the distance measured on the CPU (profiles/knn_normals_parity.json), the sign rule exactly."""
import ctypes
import json
import re

import numpy as np
import pytest

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, correspondences, formats, ops, sampling
from tests import knn_ref as kr
from tests.knn_ref import ROOT, cases, frame_clouds

f32 = np.float32
# 100 x the maxima python -m tests.knn_ref measured here on the CPU (profiles/knn_normals_parity.json): eigh's own error is of
# the same order, and the bounds only have to catch a wrong vector or an iteration that has not converged
MAX_ANGLE = 100 * 1.97206245760654e-15
MAX_CURV_REL = 100 * 1.2986172298839794e-15


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("name", list(cases()))
def test_host_rows_are_the_brute_force_rows(hip_lib, name):
    q, t, K = cases()[name]
    idx, d2 = ops.knn_host(q, t, K)
    want_idx, want_d2 = kr.brute_knn(q, t, K)
    assert idx.dtype == np.int32 and d2.dtype == f32 and idx.shape == d2.shape == (len(q), K)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(d2), bits(want_d2))
    assert ops.knn_host(q, t, K, want_d2=False)[1] is None and np.array_equal(ops.knn_host(q, t, K, want_d2=False)[0], idx)
    assert (np.diff(d2.astype(np.float64), axis=1) >= 0).all()
    if name == "all identical":
        assert (idx == np.arange(K)).all() and (d2 == 0).all()
    if name == "K = Nt":
        assert (np.sort(idx, axis=1) == np.arange(K)).all()
    if name.startswith("integer lattice"):
        centre = 62                                                              # (2, 2, 2): itself, then the three lowest
        assert idx[centre].tolist() == [62, 37, 57, 61] and d2[centre].tolist() == [0, 1, 1, 1]       # of its six neighbours
    if name == "duplicated points":
        assert idx[0].tolist()[:4] == [0, 40, 57, 62] and (d2[0, :4] == 0).all()       # a point, then its copies by index
    if name.startswith("line"):
        assert len(np.unique(bits(d2[0]))) > K // 2                              # really distinct distances, bits apart


def test_k1_is_the_lowest_index_nearest_neighbour(hip_lib):
    """K = 1 is ops.nn_batched's rule (the nearest target, the lowest index on a tie): here against the brute force on a
    lattice, where every query between two lattice points ties."""
    lattice = cases()["integer lattice, cut inside the six axis neighbours"][1]
    q = (lattice[:60] + f32(0.5)).astype(f32)                                     # cell centres: eight corners tie
    idx, d2 = ops.knn_host(q, lattice, 1)
    want = np.array([kr.d2_bits(p, lattice).argmin() for p in q])                # argmin: the first of equal minima
    assert np.array_equal(idx[:, 0], want) and (d2 == f32(0.75)).all()


def test_permuted_queries_give_permuted_rows(hip_lib):
    q, t, K = cases()["Nt = 257, K = 64"]
    perm = np.random.default_rng(0).permutation(len(q))
    a, b = ops.knn_host(q, t, K), ops.knn_host(q[perm], t, K)
    assert np.array_equal(b[0], a[0][perm]) and np.array_equal(bits(b[1]), bits(a[1][perm]))


def test_refusals(hip_lib):
    L = hip_lib
    pts = np.zeros((4, 3), f32)
    idx, d2 = np.zeros((4, 4), np.int32), np.zeros((4, 4), f32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for shape in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, 5), (4, 2000, 1025), (4, (1 << 24) + 1, 1), (-1, 4, 1)):
        assert L.isr_knn_workspace_bytes(*shape) == 0 and L.isr_last_error(), shape
    nb = L.isr_knn_workspace_bytes(4, 4, 4)
    assert nb > 0 and L.isr_knn_workspace_bytes(1 << 20, 1 << 24, 1024) >= nb
    ws = np.zeros(nb, np.uint8)
    for Nq, Nt, K, word in ((0, 4, 1, b"Nq"), (4, 0, 1, b"Nt"), (4, 4, 0, b"K"), (4, 4, 5, b"K"), (4, 2000, 1025, b"K"),
                            (4, (1 << 24) + 1, 1, b"Nt")):
        assert L.isr_knn_host(vp(pts), Nq, vp(pts), Nt, K, vp(idx), vp(d2)) == -1 and word in L.isr_last_error()
        assert L.isr_knn(vp(pts), Nq, vp(pts), Nt, K, vp(idx), vp(d2), vp(ws), nb, None) == -1 and word in L.isr_last_error()
    for args in ((None, 4, vp(pts), 4, 2, vp(idx), vp(d2)), (vp(pts), 4, None, 4, 2, vp(idx), vp(d2)),
                 (vp(pts), 4, vp(pts), 4, 2, None, vp(d2))):
        assert L.isr_knn_host(*args) == -1 and b"null" in L.isr_last_error()
        assert L.isr_knn(*args, vp(ws), nb, None) == -1 and b"null" in L.isr_last_error()
    assert L.isr_knn_host(vp(pts), 4, vp(pts), 4, 2, vp(idx), None) == 0                       # d2 is optional
    # the device entry refuses before touching a device: null workspace, short workspace
    assert L.isr_knn(vp(pts), 4, vp(pts), 4, 2, vp(idx), vp(d2), None, nb, None) == -1
    assert L.isr_knn(vp(pts), 4, vp(pts), 4, 2, vp(idx), vp(d2), vp(ws), nb - 1, None) == -1 and b"workspace" in L.isr_last_error()
    curv, frames = np.zeros((4, 3)), np.zeros((4, 3, 3))
    for fn, tail in ((L.isr_local_frames_host, ()), (L.isr_local_frames, (None,))):
        assert fn(vp(pts), 0, vp(idx), 2, 1, vp(curv), vp(frames), *tail) == -1 and b"N" in L.isr_last_error()
        assert fn(vp(pts), 4, vp(idx), 0, 1, vp(curv), vp(frames), *tail) == -1 and b"K" in L.isr_last_error()
        assert fn(vp(pts), 4, vp(idx), 1025, 1, vp(curv), vp(frames), *tail) == -1
        for hole in range(4):
            a = [vp(pts), vp(idx), vp(curv), vp(frames)]
            a[hole] = None
            assert fn(a[0], 4, a[1], 2, 1, a[2], a[3], *tail) == -1 and b"null" in L.isr_last_error()
    bad = pts.copy()
    bad[2, 1] = np.nan
    for call in (lambda: ops.knn_host(bad, pts, 2), lambda: ops.knn_host(pts, bad, 2), lambda: ops.knn_host(pts[:, :2], pts, 2),
                 lambda: ops.knn_host(pts, pts, 5), lambda: ops.knn_host(pts, pts, 0),
                 lambda: ops.local_frames_host(pts, idx[:3]), lambda: ops.local_frames_host(pts[:, :2], idx)):
        with pytest.raises(ValueError):
            call()
    cloud = np.random.default_rng(1).normal(size=(50, 3)).astype(f32)
    for poison in (np.nan, np.inf, -np.inf):                                    # unspecified rows, every index in range
        bad = cloud.copy()
        bad[7, 0] = bad[20, 2] = poison
        got = ops.knn_host(bad, bad, 13, check_finite=False)[0]
        assert got.min() >= 0 and got.max() < 50


def test_header_and_signature_table(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_knn.h").read_text(), flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(isr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(decls) == sorted(_capi.KNN_SIGNATURES) and len(decls) == 5
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_knn.h but not exported"
        assert len(_capi.KNN_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    others = (_capi.SIGNATURES, _capi.FIELD_SIGNATURES, _capi.FPS_SIGNATURES, _capi.DENSITY_SIGNATURES,
              _capi.DENSITY_DIR_SIGNATURES, _capi.RADIUS_SIGNATURES, _capi.MC_SIGNATURES)
    assert not any(set(_capi.KNN_SIGNATURES) & set(o) for o in others)
    main = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_hip.h").read_text(), flags=re.S)
    assert "isr_knn" not in main and "isr_local_frames" not in main


def test_bounds_are_100_times_the_recorded_measurement():
    doc = json.loads((ROOT / "profiles" / "knn_normals_parity.json").read_text())
    assert MAX_ANGLE == 100 * doc["max_normal_angle_rad"] and MAX_CURV_REL == 100 * doc["max_curvature_diff_rel"]
    assert sorted(doc["clouds"]) == sorted(frame_clouds())


@pytest.fixture(scope="module")
def host_frames(hip_lib):
    """name -> (points, idx, (curvatures, frames) without the sign rule, the same with it): computed once."""
    out = {}
    for name, (pts, K) in frame_clouds().items():
        idx = ops.knn_host(pts, pts, K)[0]
        out[name] = (pts, idx, ops.local_frames_host(pts, idx, disambiguate=False), ops.local_frames_host(pts, idx, disambiguate=True))
    return out


@pytest.mark.parametrize("name", list(frame_clouds()))
def test_host_frames_against_eigh(host_frames, name):
    pts, idx, (curv, frames), (curv_d, frames_d) = host_frames[name]
    w, v = kr.eigh_frames(pts, idx)
    assert ((w[:, 1] - w[:, 0]) / w[:, 2]).min() >= kr.MIN_GAP              # by the NumPy reference alone; no point left out
    worst = kr.angle(frames[:, :, 0], v[:, :, 0]).max()
    worst_curv = (np.abs(curv - w) / w[:, 2:3]).max()
    print(f"{name}: largest normal angle {worst:.3e} rad (bound {MAX_ANGLE:.3e}), curvature {worst_curv:.3e} (bound {MAX_CURV_REL:.3e})")
    assert worst <= MAX_ANGLE and worst_curv <= MAX_CURV_REL
    assert kr.angle(frames_d[:, :, 0], v[:, :, 0]).max() <= MAX_ANGLE
    assert (np.diff(curv, axis=1) >= 0).all() and np.array_equal(curv, curv_d)
    eye = np.eye(3)
    for f in (frames, frames_d):
        assert np.abs(np.einsum("nra,nrb->nab", f, f) - eye).max() <= 1e-12      # orthonormal columns
    assert np.abs(np.linalg.det(frames_d) - 1.0).max() <= 1e-12                  # right-handed with the sign rule
    assert np.abs(np.cross(frames_d[:, :, 2], frames_d[:, :, 0]) - frames_d[:, :, 1]).max() <= 1e-15


@pytest.mark.parametrize("name", ["noisy plane, K = 20", "torus, K = 20"])
def test_sign_rule_is_the_restated_count(host_frames, name):
    pts, idx, (_, frames), (_, frames_d) = host_frames[name]
    K = idx.shape[1]
    flipped = 0
    for col in (0, 2):
        flip = 2 * kr.positive_counts(pts, idx, frames[:, :, col]) < K
        want = np.where(flip[:, None], -frames[:, :, col], frames[:, :, col])
        assert np.array_equal(want, frames_d[:, :, col])                         # negation is exact
        flipped += int(flip.sum())
    assert 0 < flipped < 2 * len(pts)


def test_sign_rule_on_a_half_plane(hip_lib):
    """Points of the plane z = 0: point 0 at the origin, every other one on the side x > 0.  The neighbourhood of point 0
    is the whole cloud, its normal is +-z with no neighbour on either side (count 0: flipped to whatever is the negative of
    Jacobi's vector), and its largest direction ends up pointing to the side the neighbours are on."""
    rng = np.random.default_rng(3)
    pts = np.concatenate([np.zeros((1, 3)), np.stack([rng.uniform(0.1, 1, 40), rng.uniform(-0.2, 0.2, 40), np.zeros(40)], 1)]).astype(f32)
    idx = ops.knn_host(pts, pts, len(pts))[0]
    _, raw = ops.local_frames_host(pts, idx, disambiguate=False)
    _, out = ops.local_frames_host(pts, idx, disambiguate=True)
    assert np.array_equal(np.abs(raw[0, :, 0]), [0, 0, 1]) and np.array_equal(out[0, :, 0], -raw[0, :, 0])
    assert out[0, 0, 2] > 0.9                                                    # 40 of 41 neighbours have dx > 0
    assert np.array_equal(np.abs(out[0, :, 2]), np.abs(raw[0, :, 2]))


def test_identical_cloud_gives_the_stated_finite_frame(hip_lib):
    pts = np.tile(np.array([[0.1, 0.2, 0.3]], f32), (33, 1))
    idx = ops.knn_host(pts, pts, 7)[0]
    curv, frames = ops.local_frames_host(pts, idx, disambiguate=False)
    assert (curv == 0).all() and (frames == np.eye(3)).all()
    curv, frames = ops.local_frames_host(pts, idx, disambiguate=True)
    assert (curv == 0).all() and (frames == np.diag([-1.0, 1.0, -1.0])).all()
    one = ops.local_frames_host(pts[:1], np.zeros((1, 1), np.int32))                   # K = 1 is the same case
    assert (one[0] == 0).all() and (one[1] == np.diag([-1.0, 1.0, -1.0])).all()
    wild = ops.local_frames_host(pts, np.full((33, 7), 10 ** 6, np.int32))             # clamped, never an access outside
    assert np.isfinite(wild[1]).all()


def test_pytorch3d_call_shapes_on_the_host(hip_lib):
    torus, K = frame_clouds()["torus, K = 20"]
    idx = ops.knn_host(torus, torus, K)[0]
    curv, frames = sampling.estimate_pointcloud_local_coord_frames(torus, K, host=True)
    want = ops.local_frames_host(torus, idx)
    assert curv.dtype == frames.dtype == f32 and curv.shape == (900, 3) and frames.shape == (900, 3, 3)
    assert np.array_equal(curv, want[0].astype(f32)) and np.array_equal(frames, want[1].astype(f32))
    normals = sampling.estimate_pointcloud_normals(torus, K, host=True)
    assert np.array_equal(normals, frames[:, :, 0])
    raw = sampling.estimate_pointcloud_normals(torus, K, disambiguate_directions=False, host=True)
    assert np.array_equal(np.abs(raw), np.abs(normals))
    both = np.stack([torus[:300], torus[300:600]])
    nb = sampling.estimate_pointcloud_normals(both, 12, host=True)
    assert nb.shape == (2, 300, 3) and np.array_equal(nb[1], sampling.estimate_pointcloud_normals(both[1], 12, host=True))
    for K_bad in (0, 900, 901):
        with pytest.raises(ValueError):
            sampling.estimate_pointcloud_normals(torus, K_bad, host=True)
    with pytest.raises(ValueError):
        sampling.estimate_pointcloud_normals(torus[:, :2], 5, host=True)


def test_subsampled_normals_and_their_files(hip_lib, tmp_path):
    cloud = kr.surface_cloud("torus", 2000, 9).astype(np.float64)
    subvert, subnormal = correspondences.subsampled_normals(cloud, K=300, neighborhood_size=120, host=True)
    assert subvert.dtype == subnormal.dtype == f32 and subvert.shape == subnormal.shape == (300, 3)
    pick = ops.fps_sample_host(cloud.astype(f32), 300)[0]
    assert pick[0] == 0 and np.array_equal(subvert, cloud.astype(f32)[pick])           # FPS from index 0
    assert np.array_equal(subnormal, -sampling.estimate_pointcloud_normals(subvert, 120, host=True))
    assert np.abs(np.linalg.norm(subnormal, axis=1) - 1).max() < 1e-6
    paths = formats.save_subsampled_normals(tmp_path / "nerf", subvert, subnormal)
    assert [p.name for p in paths] == ["subvert1.npy", "subnormal1.npy"]
    assert np.load(paths[0]).dtype == f32 and np.load(paths[1]).dtype == f32
    v1, n1 = formats.load_subsampled_normals(tmp_path / "nerf")
    assert v1.dtype == n1.dtype == f32 and np.array_equal(v1, subvert) and np.array_equal(n1, subnormal)
    for kwargs in (dict(K=2001), dict(K=300, neighborhood_size=300), dict(K=300, neighborhood_size=0)):
        with pytest.raises(ValueError):
            correspondences.subsampled_normals(cloud, host=True, **kwargs)
    with pytest.raises(ValueError):
        formats.save_subsampled_normals(tmp_path / "nerf", subvert, subnormal[:10])
