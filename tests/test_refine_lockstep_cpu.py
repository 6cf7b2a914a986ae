"""CPU: the lockstep minimiser behind refine_poses (every run equals a plain scipy.optimize.minimize, the rounds are as few
as the longest run needs, a failing objective ends the call), and the batched refine objective's C-ABI argument errors."""
import ctypes
import threading

import numpy as np
import pytest
from scipy.optimize import minimize


def _problems():
    """8 NumPy problems: Rosenbrock in 2..5 dimensions and shifted / scaled quadratics, each with its own start."""
    rng = np.random.default_rng(11)
    out = []
    for d in (2, 3, 4, 5):
        x0 = rng.normal(0, 1.2, d)

        def rosen(x):
            f = float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2))
            g = np.zeros_like(x)
            g[:-1] += -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2 * (1 - x[:-1])
            g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
            return f, g
        out.append((x0, rosen))
    for d in (1, 3, 6, 8):
        A = rng.normal(size=(d, d))
        H = A @ A.T + d * np.eye(d)
        c = rng.normal(size=d)

        def quad(x, H=H, c=c):
            r = x - c
            return float(0.5 * r @ H @ r), H @ r
        out.append((rng.normal(0, 3, d), quad))
    return out


def _plain(x0, fg, method):
    pts = set()

    def fun(x):
        pts.add(np.asarray(x, np.float64).tobytes())
        return fg(np.asarray(x, np.float64))[0]

    def jac(x):
        pts.add(np.asarray(x, np.float64).tobytes())
        return fg(np.asarray(x, np.float64))[1]
    return minimize(fun, x0, jac=jac, method=method), len(pts)


@pytest.mark.parametrize("method", ["BFGS", "CG"])
def test_lockstep_equals_plain_minimize(method):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd.pose_refine import lockstep_minimize
    probs = _problems()
    calls = []

    def batch_eval(reqs):
        assert threading.current_thread() is threading.main_thread()
        assert len({k for k, _ in reqs}) == len(reqs)
        calls.append(len(reqs))
        return [probs[k][1](x) for k, x in reqs]

    res, rounds = lockstep_minimize([p[0] for p in probs], batch_eval, method=method)
    assert rounds == len(calls)
    most = 0
    for k, (x0, fg) in enumerate(probs):
        ref, n_pts = _plain(x0, fg, method)
        most = max(most, n_pts)
        r = res[k]
        assert np.array_equal(r.x, ref.x) and r.fun == ref.fun, k
        assert (r.nit, r.nfev, r.njev) == (ref.nit, ref.nfev, ref.njev), k
        assert r.success == ref.success
    assert rounds <= most
    assert sum(calls) <= sum(_plain(x0, fg, method)[1] for x0, fg in probs)


def test_lockstep_error_propagates():
    from imagesequenceregistrationfor6dposeestimationlabeling_amd.pose_refine import lockstep_minimize
    probs = _problems()
    seen = {"n": 0}

    def batch_eval(reqs):
        out = []
        for k, x in reqs:
            if k == 3:
                seen["n"] += 1
                if seen["n"] == 4:
                    raise FloatingPointError("objective of problem 3 failed")
            out.append(probs[k][1](x))
        return out

    box = {}

    def run():
        try:
            lockstep_minimize([p[0] for p in probs], batch_eval)
        except FloatingPointError as e:
            box["err"] = e

    th = threading.Thread(target=run, daemon=True)
    th.start()
    th.join(timeout=30)
    assert not th.is_alive(), "lockstep_minimize hung after a failing evaluation"
    assert "problem 3" in str(box["err"])
    before = threading.active_count()

    # an exception inside one worker's own objective (a gradient scipy cannot use) also reaches the caller, and no worker is left
    def bad_eval(reqs):
        return [(probs[k][1](x)[0], "not a gradient" if k == 5 else probs[k][1](x)[1]) for k, x in reqs]
    with pytest.raises((TypeError, ValueError)):
        lockstep_minimize([p[0] for p in probs], bad_eval)
    assert threading.active_count() <= before


def test_lockstep_no_problems():
    from imagesequenceregistrationfor6dposeestimationlabeling_amd.pose_refine import lockstep_minimize
    res, rounds = lockstep_minimize([], lambda reqs: [])
    assert res == [] and rounds == 0


def test_refine_batch_arg_errors(hip_lib):
    L = hip_lib
    assert L.isr_abi_version() == 6
    assert L.isr_refine_objective_batch_workspace_bytes(0) == 0
    assert L.isr_refine_objective_batch_workspace_bytes(3) >= 3 * 64 * 14 * 8
    offs = (ctypes.c_int32 * 3)(0, 5, 9)
    offs_p = ctypes.cast(offs, ctypes.c_void_p)
    fake = 0x1000                                      # never dereferenced: every call below fails its checks on the host

    def call(X=fake, offs_host=offs_p, n_img=2, e=12, res=16, mode=0, n_items=2, nout=4, ws=fake, ws_bytes=1 << 20):
        return L.isr_refine_objective_batch(X, fake, offs_host, fake, n_img, e, fake, fake, res, mode, fake, fake, fake,
                                            n_items, fake, nout, ws, ws_bytes, None)

    assert call(X=None) == -1 and b"null" in L.isr_last_error()
    assert call(offs_host=None) == -1 and b"null" in L.isr_last_error()
    assert call(nout=5) == -1 and b"nout" in L.isr_last_error()
    assert call(mode=3) == -1 and b"interpolation" in L.isr_last_error()
    assert call(n_items=-1) == -1 and b"n_items" in L.isr_last_error()
    assert call(n_img=0) == -1 and b"n_img" in L.isr_last_error()
    empty = (ctypes.c_int32 * 3)(0, 5, 5)               # image 1 sees nothing
    assert call(offs_host=ctypes.cast(empty, ctypes.c_void_p)) == -1 and b"image 1 has N=0" in L.isr_last_error()
    assert call(ws=None) == -2 and b"workspace" in L.isr_last_error()
    assert call(ws_bytes=100) == -2 and b"workspace" in L.isr_last_error()
    assert call(n_items=0, ws=None, ws_bytes=0) == 0          # nothing to evaluate: nothing is launched
