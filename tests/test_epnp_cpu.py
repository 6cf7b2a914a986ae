"""CPU: the EPnP solver of pnp(final="epnp") (csrc/epnp.hpp) built as host code (isr_epnp_host, ops.epnp_host) against the
truth of exact noiseless scenes and against tests/epnp_ref.py (NumPy, np.linalg, the literal M); its Jacobi stage against
np.linalg.eigh; the argument errors of the new C entries, without a device."""
import ctypes

import numpy as np
import pytest

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops, synth
from tests import epnp_ref as ref


def _noisy(seed, M=600, px=1.5, drop=0.3):
    rng = np.random.default_rng(seed)
    pts = synth.tless_like(rng, 4000)
    K = synth.camera()
    R, t = synth.random_poses(rng, 1)
    X = pts[rng.choice(len(pts), M)]
    uv = synth.project(K, R[0], t[0], X) + rng.normal(0, px, (M, 2))
    sel = rng.random(M) >= rng.uniform(0.0, drop)
    return K, R[0], t[0], X.astype(np.float32), uv.astype(np.float32), sel


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))


@pytest.mark.parametrize("n", [5, 6, 10, 100, 20000])
def test_exact_scene_recovers_truth(hip_lib, n):
    rng = np.random.default_rng(n)
    K, R, t, X, uv = ref.exact_scene(rng, n)
    Rt, err, ch = ops.epnp_host(X, uv, K)
    assert ch in (1, 2, 3)
    assert synth.rot_angle(Rt[:, :3], R) < 1e-9
    assert np.linalg.norm(Rt[:, 3] - t) < 1e-9 * np.linalg.norm(t)
    assert err[ch - 1] < 1e-6 and err[ch - 1] == err.min()


def test_exact_scene_four_points(hip_lib):
    """n = 4: M^T M has a 4-dimensional null space, which cv2's three approximations (and 5 Gauss-Newton steps) do not
    solve exactly — the pose can be far off, in the NumPy statement as well.  The host returns a finite rotation and the
    candidate with the smallest error."""
    for s in range(5):
        K, R, t, X, uv = ref.exact_scene(np.random.default_rng(100 + s), 4)
        Rt, err, ch = ops.epnp_host(X, uv, K)
        assert np.all(np.isfinite(Rt)) and ch in (1, 2, 3) and err[ch - 1] == err.min()
        assert np.max(np.abs(Rt[:, :3] @ Rt[:, :3].T - np.eye(3))) < 1e-9


@pytest.mark.parametrize("seed", range(12))
def test_noisy_matches_numpy(hip_lib, seed):
    K, R, t, X, uv, sel = _noisy(seed, px=1.0 + (seed % 2))
    Rt, err, ch = ops.epnp_host(X, uv, K, ref.mask_words(sel))
    Rr, er, cr = ref.epnp(X, uv, K, sel)
    # other factorisations (Jacobi / Householder vs LAPACK) and summation orders: 1e-8 relative
    np.testing.assert_allclose(err, er, rtol=1e-8)
    if ch != cr:   # only a tie to rounding may pick differently
        assert abs(er[ch - 1] - er[cr - 1]) <= 1e-8 * er[cr - 1]
    else:
        assert _rel(Rt, Rr) < 1e-8
    assert synth.rot_angle(Rt[:, :3], R) < 0.05


def test_mask_equals_selection(hip_lib):
    K, R, t, X, uv, sel = _noisy(77)
    a = ops.epnp_host(X, uv, K, ref.mask_words(sel))
    b = ops.epnp_host(X[sel], uv[sel], K)
    # the same points, other slots of the reduction: equal to rounding, not bit for bit
    assert a[2] == b[2] and _rel(a[0], b[0]) < 1e-12


@pytest.mark.parametrize("seed", range(5))
def test_planar_points(hip_lib, seed):
    """z = 0 object points: c3 = c0, alpha_3 = 0, and M^T M has three exactly zero rows and columns.  Its null space is
    then degenerate, so the three candidates depend on the eigenvector basis and need not agree with NumPy's (the
    approximations are not exact there); the pose returned is finite, its rotation is NumPy's and the truth's to f32
    accuracy, its translation within 0.2 %."""
    rng = np.random.default_rng(seed)
    K = synth.camera()
    R, t = synth.random_poses(rng, 1)
    X = np.concatenate([rng.uniform(-60, 60, (300, 2)), np.zeros((300, 1))], 1).astype(np.float32)
    uv = synth.project(K, R[0], t[0], X.astype(np.float64)).astype(np.float32)
    Rt, err, ch = ops.epnp_host(X, uv, K)
    Rr, er, cr = ref.epnp(X, uv, K)
    assert np.all(np.isfinite(Rt)) and np.all(np.isfinite(err))
    assert synth.rot_angle(Rt[:, :3], R[0]) < 1e-6 and synth.rot_angle(Rt[:, :3], Rr[:, :3]) < 1e-6
    assert np.linalg.norm(Rt[:, 3] - Rr[:, 3]) < 2e-3 * np.linalg.norm(Rr[:, 3]) and err[ch - 1] < 0.1


@pytest.mark.parametrize("seed", range(6))
def test_jacobi_psd(hip_lib, seed):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(12, 12)) * np.exp(rng.normal(size=12) * 2.0)
    A = G @ G.T
    w, V = ops.epnp_jacobi_host(A)
    we = np.linalg.eigvalsh(A)
    assert np.all(np.diff(w) >= 0)
    assert np.max(np.abs(w - we)) <= 1e-12 * we.max()
    assert np.max(np.abs(V.T @ V - np.eye(12))) < 1e-13
    assert np.max(np.abs(A @ V - V * w)) <= 1e-12 * we.max()


def test_argument_errors(hip_lib):
    L = hip_lib
    K = np.ascontiguousarray(synth.camera().reshape(9))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    X = np.zeros((10, 3), np.float32)
    uv = np.zeros((10, 2), np.float32)
    Rt, err, ch = np.zeros(12), np.zeros(3), ctypes.c_int32(0)
    # fewer than 4 masked points
    mk = np.array([0b111], np.uint32)
    rc = L.isr_epnp_host(vp(X), vp(uv), vp(mk), 10, vp(K), vp(Rt), vp(err), ctypes.byref(ch))
    assert rc == -1 and b"4" in L.isr_last_error()
    with pytest.raises(_capi.IsrError):
        ops.epnp_host(X[:3], uv[:3], K)
    # null pointers
    assert L.isr_epnp_host(None, vp(uv), None, 10, vp(K), vp(Rt), vp(err), ctypes.byref(ch)) == -1
    assert b"null" in L.isr_last_error()
    assert L.isr_epnp_batch(None, None, None, 16, 1, None, None, None, None, None, None, 0, None) == -1
    assert L.isr_epnp_jacobi_host(None, 3, None, None) == -1
    # final_mode of isr_pnp_ransac_batch: checked first, no device touched
    for B, fm in [(1, 7), (2, -1)]:
        rc = L.isr_pnp_ransac_batch(None, None, None, 100, B, None, 100, None, 2.0, 0.99, 10, None, None, None, None, None,
                                    None, 0, None, 0, 0, 0, fm)
        assert rc == -1 and b"final_mode" in L.isr_last_error()
    # workspace sizes: REFIT positive, EPNP larger, unknown 0
    sz = L.isr_pnp_ransac_batch_workspace_bytes
    for B in (1, 7):
        assert sz(5000, 500, B, 0) > 0
        assert sz(5000, 500, B, 1) > sz(5000, 500, B, 0)
        assert sz(5000, 500, B, 2) == 0
    assert L.isr_epnp_batch_workspace_bytes(0, 1) == 0


def test_final_keyword_checked_first():
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import registration
    with pytest.raises(ValueError, match="final"):
        ops._loop_args("sequential", "ransac", None, "bogus")
    with pytest.raises(ValueError, match="final"):
        registration.pnp(np.zeros((10, 3)), np.zeros((10, 2)), np.eye(3), final="bogus")
