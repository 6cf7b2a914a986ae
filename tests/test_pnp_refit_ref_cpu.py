"""tests/pnp_refit_ref.py stands on its own (no device): the f64 restatement of the refit against its np.longdouble twin
and against oracle/pnp_oracle.py:refine at convergence, the retraction, and the exits that keep the pose.

Measured here (x86-64, 80-bit long double), refine against refine_ext over 1, 2, 3 and 10 iterations, rotation in rad /
translation relative to |t| + 1, with the object at 700 mm: at most 2.1e-12 / 5.6e-13 (5 correspondences, 10 iterations;
4 correspondences: 1.3e-12; from 31 correspondences up at most 5.7e-13 / 3.8e-14, and as low as 6.5e-17 by luck).  At 10
iterations most of it is what the stopping rule leaves undone (the twin runs on), not rounding.  rr.FLOOR_ROT /
rr.FLOOR_TRANS, the floor of the device tests' tolerance, is that maximum rounded up; this module asserts that no case at
700 mm exceeds it.  6 m away: at most 6.4e-12 / 1.9e-12 (one iteration from 15 degrees), held to a hundredth of the cap."""
import numpy as np
import pytest

from imagesequenceregistrationfor6dposeestimationlabeling_amd import synth
from oracle import pnp_oracle as po
from tests import pnp_refit_ref as rr

# kind, seed, M, start (deg, mm)
CASES = [("few", 1, 4, 1.5, 1.5), ("few", 2, 5, 1.5, 1.5), ("few", 3, 6, 1.5, 1.5), ("general", 4, 31, 1.5, 1.5),
         ("general", 5, 64, 1.5, 1.5), ("general", 6, 257, 1.5, 1.5), ("general", 7, 8193, 1.5, 1.5),
         ("planar", 9, 4, 1.5, 1.5), ("planar", 10, 6, 1.5, 1.5), ("planar", 11, 300, 1.5, 1.5), ("far", 12, 300, 1.5, 1.5),
         ("far", 13, 6, 1.5, 1.5), ("general", 20, 300, 15.0, 20.0), ("planar", 21, 300, 15.0, 20.0), ("far", 22, 300, 15.0, 20.0)]


def _args(s):
    return s["p3d"], s["p2d"], s["K"]


@pytest.mark.skipif(not rr.HAS_EXT, reason="np.longdouble is no wider than f64 here: no extended twin to compare with")
@pytest.mark.parametrize("kind,seed,M,deg,mm", CASES)
def test_refine_against_extended_twin(kind, seed, M, deg, mm):
    s, sel, Rt0 = rr.refine_case(kind, seed, M, deg, mm)
    for iters in (1, 2, 3, 10):
        da, dt = rr.d_ref(s, sel, Rt0, iters)
        print(f"[{kind} seed {seed} M {M} start {deg} deg iters {iters}] d_ref {da:.2e} rad {dt:.2e} rel")
        # the object at 700 mm: the floor; 6 m away J^T J is 1e4 times worse conditioned, and 100 * d_ref must still fit the cap
        lim = (rr.CAP_ROT / 100, rr.CAP_TRANS / 100) if kind == "far" else (rr.FLOOR_ROT, rr.FLOOR_TRANS)
        assert da <= lim[0] and dt <= lim[1], (kind, seed, M, iters, da, dt)
    # both reach the final cost in 3 iterations from the small start (quadratic convergence)
    if deg < 2:
        c3, c10 = (rr.cost(*_args(s), rr.refine(*_args(s), Rt0, sel, it), sel) for it in (3, 10))
        assert abs(c3 - c10) <= 1e-9 * c10


@pytest.mark.parametrize("kind,seed,M,deg,mm", CASES)
def test_refine_against_oracle_at_convergence(kind, seed, M, deg, mm):
    """Rodrigues or the quaternion retraction: the same fixed point."""
    s, sel, Rt0 = rr.refine_case(kind, seed, M, deg, mm)
    a, b = rr.refine(*_args(s), Rt0, sel, 10), po.refine(*_args(s), Rt0, sel, 10)
    da, dt = rr.pose_dist(a, b)
    assert da < 1e-10 and dt < 1e-10, (da, dt)
    assert rr.grad_norm(*_args(s), a, sel) < 1e-11


def test_partial_counts_differ_from_rodrigues_by_the_cube():
    """Why po.refine is no reference below convergence: after ONE step from 15 degrees the two retractions are
    O(|w|^3) apart, far above the tolerance of the device tests."""
    s, sel, Rt0 = rr.refine_case("general", 20, 300, 15.0, 20.0)
    a, b = rr.refine(*_args(s), Rt0, sel, 1), po.refine(*_args(s), Rt0, sel, 1)
    w = np.linalg.norm(rr.gn_step(*_args(s), Rt0, sel)[0][:3])
    assert 1e-6 < rr.pose_dist(a, b)[0] < w ** 3


def test_retract():
    rng = np.random.default_rng(3)
    Rt = rr.general(3, 8)["Rt"]
    for mag in (1e-9, 1e-4, 1e-2, 0.3, 2.0):
        w = rng.normal(size=3)
        dx = np.concatenate([mag * w / np.linalg.norm(w), rng.normal(size=3)])
        T = rr.retract(Rt, dx)
        R = T[:, :3]
        assert abs(np.linalg.det(R) - 1) < 1e-14 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
        Q = po._rodrigues(dx[:3])
        # tan(theta / 2) = |w| / 2 against theta = |w|: the angles differ by |w|^3 / 12 + O(|w|^5), the axis is shared
        assert synth.rot_angle(R, Q @ Rt[:, :3]) <= mag ** 3 / 12 * 1.01 + 1e-15
        assert np.allclose(T[:, 3], R @ Rt[:, :3].T @ Rt[:, 3] + dx[3:], rtol=0, atol=1e-12 * np.abs(Rt[:, 3]).max())
    assert np.array_equal(rr.retract(Rt, np.zeros(6)), Rt)


def test_exits_return_their_input_bit_for_bit():
    s, sel, Rt0 = rr.refine_case("general", 5, 64)
    same = lambda a, b: np.array_equal(a.view(np.int64), b.view(np.int64))
    three = np.zeros(64, bool)
    three[[3, 17, 40]] = True
    for few_sel in (np.zeros(64, bool), three, np.array([3, 17, 40])):
        assert same(rr.refine(*_args(s), Rt0, few_sel, 10), Rt0)
    assert same(rr.refine(*_args(s), Rt0, sel, 0), Rt0)
    # a selected correspondence with a NaN coordinate: the sums are NaN, the pose stays
    bad = s["p3d"].copy()
    bad[np.nonzero(sel)[0][5], 1] = np.nan
    assert rr.gn_step(bad, s["p2d"], s["K"], Rt0, sel)[0] is None
    assert same(rr.refine(bad, s["p2d"], s["K"], Rt0, sel, 10), Rt0)
    # unselected rows may hold anything
    junk = s["p3d"].copy()
    junk[~sel] = np.nan
    assert same(rr.refine(junk, s["p2d"], s["K"], Rt0, sel, 10), rr.refine(*_args(s), Rt0, sel, 10))
    # ... and one exactly in the camera's plane z_c = 0 under the start pose (1 / 0)
    z, zsel, zRt0, m = rr.zc0_case(7, 64)
    assert zsel[m] and (z["p3d"][m].astype(np.float64) @ zRt0[2, :3] + zRt0[2, 3]) == 0.0
    assert rr.gn_step(*_args(z), zRt0, zsel)[0] is None
    assert same(rr.refine(*_args(z), zRt0, zsel, 10), zRt0)
    zsel[m] = False                                             # without it the case is an ordinary one
    assert rr.pose_dist(rr.refine(*_args(z), zRt0, zsel, 10), z["Rt"])[0] < 3e-2


def test_collinear_points_are_a_singular_system():
    """Exactly collinear in f32: the scaled J^T J has an eigenvalue of rounding size at any pose and no step is taken —
    while the well-posed families keep every relative Cholesky pivot well above PIVOT_REL (measured: >= 9.7e-5 at 700 mm,
    3.9e-6 for 6 correspondences 6 m away)."""
    for seed, M in ((60, 300), (61, 6)):
        s, sel, Rt0 = rr.refine_case("collinear", seed, M)
        X = s["p3d"].astype(np.float64)
        assert not np.any(np.cross(X - X[0], np.array([1.5, -1.0, 0.5]))) and len(np.unique(X, axis=0)) >= 4
        JtJ = rr.gn_step(*_args(s), Rt0, sel)[1]
        ev = np.linalg.eigvalsh(JtJ / np.sqrt(np.outer(np.diag(JtJ), np.diag(JtJ))))
        assert abs(ev[0]) < 1e-13
        assert rr.gn_step(*_args(s), Rt0, sel)[0] is None
        assert np.array_equal(rr.refine(*_args(s), Rt0, sel, 10), Rt0)
    for kind, seed, M, deg, mm in CASES:
        s, sel, Rt0 = rr.refine_case(kind, seed, M, deg, mm)
        JtJ = rr.gn_step(*_args(s), Rt0, sel)[1]
        piv = np.diag(np.linalg.cholesky(JtJ)) ** 2 / np.diag(JtJ)
        print(f"[{kind} seed {seed} M {M}] smallest relative pivot {piv.min():.2e}")
        assert piv.min() > 100 * rr.PIVOT_REL


def test_chain_orders_refits_and_masks(oracle_lib):
    s = rr.general(31, 400, 0.3, 0.3)
    Rt0 = rr.start_pose(5, s["Rt"], 0.5, 0.5)
    inl0 = rr.mask_of(*_args(s), Rt0, 2.0, oracle_lib)
    pose, fin, mid = rr.chain(*_args(s), Rt0, np.nonzero(inl0)[0], 10, 2.0, oracle_lib)
    p1 = rr.refine(*_args(s), Rt0, inl0, 10)
    assert np.array_equal(mid, rr.mask_of(*_args(s), p1, 2.0, oracle_lib))
    assert np.array_equal(pose, rr.refine(*_args(s), p1, mid, 10))
    assert np.array_equal(fin, rr.mask_of(*_args(s), pose, 2.0, oracle_lib))
    assert fin.sum() > 0.9 * s["inl"].sum() and rr.pose_dist(pose, s["Rt"])[0] < 3e-3
