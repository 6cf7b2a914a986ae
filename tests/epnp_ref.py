"""A NumPy statement of the EPnP solver of csrc/epnp.hpp, written from the same seven steps with np.linalg (eigh, svd,
lstsq) and the literal 2n x 12 matrix M, for tests/test_epnp_cpu.py.  Not bit-exact with the header (other
factorisations, other summation orders): it checks the algorithm, the header's host build checks the device."""
import numpy as np


def _pinv_cut(CC):
    U, s, Vt = np.linalg.svd(CC)
    tol = 2.0 * np.finfo(np.float64).eps * s.sum()
    inv = np.where(s > tol, 1.0 / np.where(s > tol, s, 1.0), 0.0)
    return Vt.T @ np.diag(inv) @ U.T


def _L_rho(v, cws):
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    L = np.zeros((6, 10))
    rho = np.zeros(6)
    for p, (a, b) in enumerate(pairs):
        dv = [v[i].reshape(4, 3)[a] - v[i].reshape(4, 3)[b] for i in range(4)]
        d = lambda i, j: float(dv[i] @ dv[j])
        L[p] = [d(0, 0), 2 * d(0, 1), d(1, 1), 2 * d(0, 2), 2 * d(1, 2), d(2, 2), 2 * d(0, 3), 2 * d(1, 3), 2 * d(2, 3), d(3, 3)]
        rho[p] = float(np.sum((cws[a] - cws[b]) ** 2))
    return L, rho


def _gauss_newton(L, rho, be):
    be = be.copy()
    for _ in range(5):
        b0, b1, b2, b3 = be
        A = np.stack([2 * L[:, 0] * b0 + L[:, 1] * b1 + L[:, 3] * b2 + L[:, 6] * b3,
                      L[:, 1] * b0 + 2 * L[:, 2] * b1 + L[:, 4] * b2 + L[:, 7] * b3,
                      L[:, 3] * b0 + L[:, 4] * b1 + 2 * L[:, 5] * b2 + L[:, 8] * b3,
                      L[:, 6] * b0 + L[:, 7] * b1 + L[:, 8] * b2 + 2 * L[:, 9] * b3], axis=1)
        quad = np.array([b0 * b0, b0 * b1, b1 * b1, b0 * b2, b1 * b2, b2 * b2, b0 * b3, b1 * b3, b2 * b3, b3 * b3])
        r = rho - L @ quad
        be = be + np.linalg.lstsq(A, r, rcond=None)[0]
    return be


def _betas(L, rho):
    out = []
    x = np.linalg.lstsq(L[:, [0, 1, 3, 6]], rho, rcond=None)[0]
    b0 = np.sqrt(abs(x[0]))
    s = -1.0 if x[0] < 0 else 1.0
    out.append(np.array([b0, s * x[1] / b0, s * x[2] / b0, s * x[3] / b0]))
    for cols in ([0, 1, 2], [0, 1, 2, 3, 4]):
        x = np.linalg.lstsq(L[:, cols], rho, rcond=None)[0]
        if x[0] < 0:
            b0, b1 = np.sqrt(-x[0]), (np.sqrt(-x[2]) if x[2] < 0 else 0.0)
        else:
            b0, b1 = np.sqrt(x[0]), (np.sqrt(x[2]) if x[2] > 0 else 0.0)
        if x[1] < 0:
            b0 = -b0
        b2 = x[3] / b0 if len(cols) == 5 else 0.0
        out.append(np.array([b0, b1, b2, 0.0]))
    return [_gauss_newton(L, rho, b) for b in out]


def _procrustes(pcs, P):
    pc0, pw0 = pcs.mean(0), P.mean(0)
    B = (pcs - pc0).T @ (P - pw0)
    _, s, Vt = np.linalg.svd(B)
    v1, v2 = Vt[0], Vt[1]
    v3 = np.cross(v1, v2)
    u1, u2 = B @ v1 / s[0], B @ v2 / s[1]
    u3 = (-1.0 if np.linalg.det(B) < 0 else 1.0) * np.cross(u1, u2)
    R = np.stack([u1, u2, u3], 1) @ np.stack([v1, v2, v3], 1).T
    if np.linalg.det(R) < 0:
        R[2] = -R[2]
    return R, pc0 - R @ pw0


def epnp(p3d, p2d, K, mask=None):
    """p3d (M, 3), p2d (M, 2), K (3, 3), mask (M,) bool or None -> (Rt (3, 4), rep_err (3,), chosen 1..3)."""
    P = np.asarray(p3d, np.float64)
    UV = np.asarray(p2d, np.float64)
    if mask is not None:
        P, UV = P[mask], UV[mask]
    K = np.asarray(K, np.float64).reshape(3, 3)
    fu, fv, uc, vc = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    n = len(P)
    # 1. control points
    c0 = P.mean(0)
    D = P - c0
    w, E = np.linalg.eigh(D.T @ D)
    order = np.argsort(-w, kind="stable")
    E = E * np.where(E[np.argmax(np.abs(E), 0), np.arange(3)] < 0, -1.0, 1.0)   # largest component positive
    cws = [c0] + [c0 + np.sqrt(max(w[i], 0.0) / n) * E[:, i] for i in order]
    # 2. barycentric coordinates
    CC = np.stack([cws[i] - cws[0] for i in (1, 2, 3)], 1)
    a123 = D @ _pinv_cut(CC).T
    al = np.concatenate([1.0 - a123.sum(1, keepdims=True), a123], 1)
    # 3. M^T M from the literal M
    M = np.zeros((2 * n, 12))
    for j in range(4):
        M[0::2, 3 * j] = al[:, j] * fu
        M[0::2, 3 * j + 2] = al[:, j] * (uc - UV[:, 0])
        M[1::2, 3 * j + 1] = al[:, j] * fv
        M[1::2, 3 * j + 2] = al[:, j] * (vc - UV[:, 1])
    # 4. null space
    _, Vm = np.linalg.eigh(M.T @ M)
    v = [Vm[:, i] for i in range(4)]
    # 5. candidates
    L, rho = _L_rho(v, cws)
    Rts, errs = [], []
    for be in _betas(L, rho):
        ccs = sum(be[i] * v[i] for i in range(4)).reshape(4, 3)
        pcs = al @ ccs
        if pcs[0, 2] < 0:             # 6. sign rule, Procrustes
            ccs, pcs = -ccs, -pcs
        R, t = _procrustes(pcs, P)
        Xc = P @ R.T + t              # 7. reprojection error
        ue = uc + fu * Xc[:, 0] / Xc[:, 2]
        ve = vc + fv * Xc[:, 1] / Xc[:, 2]
        errs.append(float(np.mean(np.sqrt((UV[:, 0] - ue) ** 2 + (UV[:, 1] - ve) ** 2))))
        Rts.append(np.concatenate([R, t[:, None]], 1))
    N = 0
    if errs[1] < errs[N]:
        N = 1
    if errs[2] < errs[N]:
        N = 2
    return Rts[N], np.array(errs), N + 1


def mask_words(sel):
    """(M,) bool -> (ceil(M / 32),) uint32 words, bit m of word m // 32."""
    sel = np.asarray(sel, bool)
    pad = np.zeros(((len(sel) + 31) // 32) * 32, bool)
    pad[: len(sel)] = sel
    bits = pad.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return bits.sum(1).astype(np.uint32)


def exact_scene(rng, n, perm=None):
    """A noiseless scene whose f32 values are exact: K = [[512, 0, 320], [0, 512, 240], [0, 0, 1]], integer pixels, dyadic
    depths, a signed-permutation rotation and a dyadic translation -> (K, R, t, p3d f32, p2d f32)."""
    K = np.array([[512.0, 0, 320.0], [0, 512.0, 240.0], [0, 0, 1.0]])
    a = rng.integers(-256, 257, n).astype(np.float64)
    b = rng.integers(-192, 193, n).astype(np.float64)
    Z = 1.0 + rng.integers(0, 257, n) / 256.0
    Xc = np.stack([a * Z / 512.0, b * Z / 512.0, Z], 1)
    if perm is None:
        perm = rng.permutation(3)
    R = np.zeros((3, 3))
    R[np.arange(3), perm] = rng.choice([-1.0, 1.0], 3)
    if np.linalg.det(R) < 0:
        R[0] = -R[0]
    t = np.array([rng.integers(-64, 65) / 256.0, rng.integers(-64, 65) / 256.0, 1.0 + rng.integers(0, 65) / 256.0])
    X = (Xc - t) @ R                 # R^T (Xc - t), exact: a signed permutation
    p2d = np.stack([a + 320.0, b + 240.0], 1)
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
    return K, R, t, X.astype(np.float32), p2d.astype(np.float32)
