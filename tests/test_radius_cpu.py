"""CPU: isr_radius_count_host (csrc/radius_count.hpp compiled for the host) against a brute-force NumPy count that uses the
same f32 fmaf chain, on the shapes where the cell grid can go wrong."""
import numpy as np
import pytest

from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
from tests import back_march_ref as br
from tests.back_march_ref import clouds

f32 = np.float32


@pytest.mark.parametrize("cap", [0, 1, 21])
@pytest.mark.parametrize("name", list(clouds()))
def test_host_count_is_the_brute_force_count(hip_lib, name, cap):
    pts, r = clouds()[name]
    got = ops.radius_count_host(pts, r, cap)
    want = br.brute_count(pts, r, cap)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if cap == 0:
        assert got.min() >= 1                       # a point finds itself
        full = {"one point": [1], "two points at exactly r": [2, 2], "two points past r": [1, 1]}.get(name)
        if full:
            assert got.tolist() == full
        if name == "all identical":
            assert (got == 33).all()
        if name == "integer lattice":
            assert got.max() == 7 and got.min() == 4            # the six axis neighbours at d2 == r2, corners have three
        if name == "three clusters":
            assert got.max() > 21 and got.min() < 21


def test_order_of_the_points_does_not_show(hip_lib):
    pts, r = clouds()["three clusters"]
    perm = np.random.default_rng(0).permutation(len(pts))
    assert np.array_equal(ops.radius_count_host(pts[perm], r)[np.argsort(perm)], ops.radius_count_host(pts, r))


def test_outlier_rule_on_coincident_clusters(hip_lib):
    """Open3D's rule as far as known (unpinned): keep a point with MORE than nb_points within the radius, itself included.
    21 coincident points keep, 20 drop.  (radius_outlier_mask itself runs on the device: tests/test_gpu_radius.py.)"""
    pts = np.concatenate([np.zeros((21, 3)), np.ones((20, 3))]).astype(f32)
    keep = ops.radius_count_host(pts, 0.05, cap=21) > 20
    assert keep[:21].all() and not keep[21:].any()


def test_refusals(hip_lib):
    import ctypes
    L = hip_lib
    pts = np.zeros((4, 3), f32)
    out = np.zeros(4, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.isr_radius_workspace_bytes(0) == 0 and L.isr_last_error()
    nb = L.isr_radius_workspace_bytes(4)
    assert nb > 0 and L.isr_radius_workspace_bytes(1 << 20) > nb
    for r in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e300):
        assert L.isr_radius_count_host(vp(pts), 4, r, 0, vp(out)) == -1 and b"radius" in L.isr_last_error()
        assert L.isr_radius_count(vp(pts), 4, r, 0, vp(out), vp(pts), nb, None) == -1
    assert L.isr_radius_count_host(vp(pts), 0, 0.1, 0, vp(out)) == -1
    assert L.isr_radius_count_host(None, 4, 0.1, 0, vp(out)) == -1 and b"null" in L.isr_last_error()
    assert L.isr_radius_count_host(vp(pts), 4, 0.1, 0, None) == -1
    # the device entry refuses before touching a device: null workspace, short workspace
    assert L.isr_radius_count(vp(pts), 4, 0.1, 0, vp(out), None, nb, None) == -1
    assert L.isr_radius_count(vp(pts), 4, 0.1, 0, vp(out), vp(pts), nb - 1, None) == -1 and b"workspace" in L.isr_last_error()
    bad = pts.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        ops.radius_count_host(bad, 0.1)
    with pytest.raises(ValueError):
        ops.radius_count_host(pts[:, :2], 0.1)
    with pytest.raises(ValueError):
        ops.radius_count_host(pts, 0.0)
    assert ops.radius_count_host(bad, 0.1, check_finite=False).shape == (4,)       # unspecified counts, no access outside
