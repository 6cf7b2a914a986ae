"""CPU: oracle.refine_pose_oracle.objective_full (the f64 reference of isr_refine_objective_full's 13 outputs) against the
oracle's own `objective` (value, d/dt) and against f64 central differences of its value (d/dR)."""
import numpy as np
import pytest
import torch

from oracle import refine_pose_oracle as rpo


def _crop(seed, res=24, e=4, N=300):
    """A smooth synthetic crop: a bumpy patch seen from ~400 mm, every sample at least 4 pixels inside the image (the
    bicubic interpolant is C1 there, so central differences converge at h^2)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1, 1, (N, 2))
    X = np.stack([6 * u[:, 0], 6 * u[:, 1], 3* np.sin(3 * u[:, 0]) * np.cos(2 * u[:, 1])], 1)
    keys = rng.normal(0, 1, (N, e))
    yy, xx = np.mgrid[0:res, 0:res] / res
    q = np.stack([np.sin(2 * np.pi * (xx * (c + 1) + yy * (e - c)) / 2) for c in range(e)], -1)
    den = np.log(1 + np.exp(np.sin(3 * xx) + np.cos(2 * yy)))[..., None]
    K = np.array([[300.0, 0, res / 2 - 0.5], [0, 300.0, res / 2 - 0.5], [0, 0, 1]])
    th = 0.3
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]])
    t = np.array([rng.normal(0, 0.5), rng.normal(0, 0.5), 400.0 + rng.normal(0, 5)])
    as_t = lambda a: torch.from_numpy(np.asarray(a, np.float64))                              # noqa: E731
    return as_t(X), as_t(keys), as_t(q), as_t(den), K, R, t


@pytest.mark.parametrize("mode", ["bilinear", "nearest", "bicubic"])
def test_objective_full_value_and_dt_equal_objective(mode):
    X, keys, q, den, K, R, t = _crop(1)
    Rt = np.concatenate([R, t[:, None]], 1)
    v, gt, gR = rpo.objective_full(Rt, X, keys, q, den, K, mode)
    v0, g0 = rpo.objective(t, R, X, keys, q, den, K, return_grad=True, interpolation=mode, dtype=torch.float64)
    assert gt.shape == (3,) and gR.shape == (9,) and gt.dtype == gR.dtype == np.float64
    # the same statements on the same operands: only the order of autograd's accumulation may differ
    assert abs(v - v0) <= 1e-14 * max(1.0, abs(v0))
    np.testing.assert_allclose(gt, g0, rtol=1e-12, atol=1e-15)
    if mode == "nearest":
        assert np.all(gt == 0) and np.all(gR == 0)
    else:
        assert np.abs(gt).max() > 1e-4 and np.abs(gR).min() > 1e-6


def test_objective_full_dR_equals_central_differences_bicubic():
    """d score / d R, row-major, by central differences of the f64 value at h = 1e-5 on every entry of R (a free 3x3: no
    Rodrigues).  Error budget relative to max|g|: truncation h^2/6 * |f'''| with d(pixel)/dR <= f * |X| / z = 300 * 9 / 400
    ~ 7 pixels per unit and image derivatives below 1 per pixel^k gives ~ 1e-10 * 7^3 / 6 ~ 6e-9; rounding eps * |f| / h
    ~ 1e-11.  1e-7 * max|g| leaves one order for the kinks of the interpolant's second derivative at pixel boundaries."""
    X, keys, q, den, K, R, t = _crop(2)
    Rt = np.concatenate([R, t[:, None]], 1)
    cam = X.numpy() @ R.T + t
    uv = (cam @ K.T)[:, :2] / cam[:, 2:]
    assert uv.min() > 4 and uv.max() < q.shape[0] - 5
    _, gt, gR = rpo.objective_full(Rt, X, keys, q, den, K, "bicubic")
    h = 1e-5
    num = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            d = np.zeros((3, 4))
            d[r, c] = h
            num[r, c] = (rpo.objective_full(Rt + d, X, keys, q, den, K, "bicubic")[0]
                         - rpo.objective_full(Rt - d, X, keys, q, den, K, "bicubic")[0]) / (2 * h)
    scale = np.abs(gR).max()
    np.testing.assert_allclose(gR, num[:, :3].reshape(9), rtol=0, atol=1e-7 * scale)
    np.testing.assert_allclose(gt, num[:, 3], rtol=0, atol=1e-7 * scale)
    # row-major: entry 3 * j + k is d/dR[j, k] — a transposed layout differs by far more than the tolerance
    assert np.abs(gR.reshape(3, 3) - gR.reshape(3, 3).T).max() > 1e-3 * scale
