"""Plain f64 reference of the correspondence matrices (test infrastructure; NumPy, no device).

The element every route writes is  log_softmax_n <Q[p], K[n]>  (isr_corr_logsoftmax, isr_ep_corr_matrices,
isr_ep_patch_corr, isr_ep_patch_corr_cells), followed by a 3 x 3 spatial max (isr_ep_pool_corr, or fused) or by the
per-block centre / block maximum of the per-pixel variant.  Here: f64 logits from the f32 (or bf16-widened) inputs, a
max-shifted log-sum-exp, and the poolings as array slices.

`bound` is the per-element error an f32 route may show against that reference, DERIVED from the kernels' arithmetic:

    u = 2^-24, g = (D + 1) u, S[p, n] = sum_d |Q[p, d] K[n, d]|, w = the f64 softmax
    bound[p, n] = g S[p, n] + g sum_n' w[p, n'] S[p, n'] + 8 u max(1, |lse[p]|, |logit[p, n]|)

    g S                 the D roundings of the k-ordered fmaf chain from 0 (gamma_D = D u / (1 - D u) <= (D + 1) u)
    g sum w S           d lse / d logit[n'] = w[n']: the first-order effect of those roundings on the row's lse
    8 u max(...)        the lse's own f32 rounding, the final subtraction's, and the exp / log ulps (K1 merges its partial
                        sums in f64)

A pooled, centre or block-maximum element gets the largest bound of its window (max is 1-Lipschitz in the sup norm).
bf16 inputs: the reference is formed from the bf16 values themselves, so nothing changes.

The `mut` arguments restate single bugs a kernel could have (tests/test_corr_matrix_ref_cpu.py shows that the comparison
catches each of them on every case the GPU tests run); mut=None is the reference."""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
KEY_BLOCK = 256          # keys per workgroup of the row kernels
SWEEP_CAP = 5e-5         # the most the three-sweep / cells constant may ever be (what the suite asserted before)

LSM_MUTATIONS = ("lse_next_row", "drop_last_key", "drop_block_key", "key_prev")
POOL_MUTATIONS = ("pool_shift_x", "pool_pad_zero")
PATCH_MUTATIONS = ("centre_low", "trailing")


def widen(x) -> np.ndarray:
    """f64 copy of an f32 / bf16 array (NumPy or host torch)."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)


def logits(Q, K) -> np.ndarray:
    return widen(Q) @ widen(K).T


def lse_rows(L: np.ndarray) -> np.ndarray:
    if L.shape[1] == 0:
        return np.full(L.shape[0], -np.inf)
    m = L.max(axis=1)
    return m + np.log(np.exp(L - m[:, None]).sum(axis=1))


def parts(Q, K, mut: str | None = None):
    """-> (out, logit, lse, w): out = logit - lse row-wise; w = the softmax (of the unmutated row)."""
    L = logits(Q, K)
    N = L.shape[1]
    lse = lse_rows(L)
    w = np.exp(L - lse[:, None])
    used = lse
    if mut == "drop_last_key":                      # the last key is left out of every lse
        used = lse_rows(L[:, :N - 1])
    elif mut == "drop_block_key":                   # the first (N % 256 == 1: the lone) key of the last key block is left out
        j = KEY_BLOCK * ((N - 1) // KEY_BLOCK)
        used = lse_rows(np.delete(L, j, axis=1))
    elif mut == "lse_next_row":                     # row p takes the lse of row p + 1
        used = np.roll(lse, -1)
    with np.errstate(invalid="ignore"):
        out = L - used[:, None]
    if mut == "key_prev":                           # key n is taken at index n - 1
        out = np.roll(out, 1, axis=1)
    return out, L, lse, w


def log_softmax(Q, K, mut: str | None = None) -> np.ndarray:
    return parts(Q, K, mut)[0]


def bound(Q, K, lse, w) -> np.ndarray:
    Q, K = widen(Q), widen(K)
    D = Q.shape[1]
    g = (D + 1) * U
    S = np.abs(Q) @ np.abs(K).T
    L = Q @ K.T
    scale = np.maximum(1.0, np.maximum(np.abs(lse)[:, None], np.abs(L)))
    return g * S + g * (w * S).sum(axis=1)[:, None] + 8 * U * scale


def matrix(Q, K, mut: str | None = None):
    """-> (out, bound) of the plain matrix."""
    out, L, lse, w = parts(Q, K, mut if mut in LSM_MUTATIONS else None)
    return out, bound(Q, K, lse, w)


def pool3(mat: np.ndarray, res: int, mut: str | None = None) -> np.ndarray:
    """3 x 3 spatial max over the pixels inside the res x res grid of a (res^2, m) matrix; outside acts as -inf."""
    m = mat.shape[1]
    pad = 0.0 if mut == "pool_pad_zero" else -np.inf
    sx = 1 if mut == "pool_shift_x" else 0
    g = np.full((res + 2, res + 3, m), pad, dtype=mat.dtype)
    g[1:res + 1, 1:res + 1] = mat.reshape(res, res, m)
    out = np.full((res, res, m), -np.inf, dtype=mat.dtype)
    for dy in range(3):
        for dx in range(3):
            np.maximum(out, g[dy:dy + res, dx + sx:dx + sx + res], out=out)
    return out.reshape(res * res, m)


def patch(query_img, keys, scale: int, mut: str | None = None):
    """avg_queries=False: per-pixel log-softmax over the res*scale x res*scale pixels (res = r // scale, trailing pixels
    unused) -> (centre, blockmax, centre_bound, blockmax_bound), each (res^2, m)."""
    qi = widen(query_img)
    r, e = qi.shape[0], qi.shape[-1]
    res = r // scale
    R = res * scale
    o = r % scale if mut == "trailing" else 0      # the blocks start at the trailing pixels' offset
    q = qi[o:o + R, o:o + R].reshape(R * R, e)
    out, bnd = matrix(q, keys, mut)
    m = out.shape[1]
    off = (scale - 1) // 2 if mut == "centre_low" else scale // 2
    out = out.reshape(res, scale, res, scale, m)
    bnd = bnd.reshape(res, scale, res, scale, m)
    n = res * res
    return (out[:, off, :, off].reshape(n, m), out.max(axis=(1, 3)).reshape(n, m),
            bnd[:, off, :, off].reshape(n, m), bnd.max(axis=(1, 3)).reshape(n, m))


def excess(got, ref, bnd) -> float:
    """max(|got - ref| - bound); inf when got holds a NaN."""
    got = widen(got)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - ref) - bnd
    return float("inf") if np.isnan(d).any() else float(d.max())


def ratio(got, ref, bnd) -> float:
    """max(|got - ref| / bound)."""
    got = widen(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - ref)
        q = np.where(d == 0, 0.0, d / bnd)
    return float("inf") if np.isnan(q).any() else float(q.max())


def compare(got, ref, bnd) -> bool:
    """|got - ref| <= bound, element for element, nothing excused."""
    return excess(got, ref, bnd) <= 0.0


# ------------------------------------------------------------------------------------------------ inputs
# Row kinds, in this order for as many rows as the case has; the remaining rows are planted at random keys.
ROW_KINDS = ("win_last", "win_0", "zero", "plus60", "minus60", "win_255", "win_256", "negzero")


def make_inputs(P: int, N: int, D: int, bf16: bool = False):
    """(Q (P, D), K (N, D)) f32 (bf16=True: values that bf16 holds exactly).
    Keys: rows of norm 3 in columns 1.., column 0 = 1 + 0.01 z — so a query's column 0 shifts all of its logits together:
    the rows `plus60` / `minus60` have every logit near +-60 with a spread of a few units.  Planted rows are 1.5 K[key]
    (`win_last`: 0.3 K[N - 1], a soft row in which every key weighs in the lse — the one row of a P = 1 case);
    `zero` is the zero query (every element -log N); `negzero` carries -0.0 entries (so does key 5); two keys are
    duplicates of non-neighbouring ones (N >= 8)."""
    rng = np.random.default_rng(1000003 * P + 1009 * N + D + (7 if bf16 else 0))
    K = rng.normal(0, 1, (N, D))
    if D > 1:
        K[:, 1:] *= 3.0 / np.maximum(np.linalg.norm(K[:, 1:], axis=1, keepdims=True), 1e-3)
    K[:, 0] = 1.0 + 0.01 * rng.normal(0, 1, N)
    if N >= 8:
        K[N - 3] = K[2]
        K[N // 2 + 1] = K[1]
        K[5, 1::2] = -0.0
    gt = rng.integers(N, size=P)
    Q = 1.5 * K[gt] + 0.3 * rng.normal(0, 1, (P, D)) / np.sqrt(D)
    Q[:, 0] = rng.normal(0, 1, P) + np.where(rng.uniform(size=P) < 0.5, -3.0, 3.0)     # |q0| >= ~1: D = 1 rows keep a spread
    for i, kind in enumerate(ROW_KINDS[:P]):
        if kind.startswith("win_"):
            j = N - 1 if kind == "win_last" else min(int(kind[4:]), N - 1)
            Q[i] = (0.3 if kind == "win_last" else 1.5) * K[j]     # win_last: a soft row, every key weighs in its lse
            Q[i, 0] = 3.0 + 0.1 * i
        elif kind == "zero":
            Q[i] = 0.0
        elif kind in ("plus60", "minus60"):
            Q[i] = 0.1 * (K[0] - K[N - 1]) + 0.2 * rng.normal(0, 1, D) / np.sqrt(D)     # a spread even between two keys
            Q[i, 0] = 60.0 if kind == "plus60" else -60.0
        elif kind == "negzero":
            Q[i, 1::3] = -0.0
    Q, K = Q.astype(np.float32), K.astype(np.float32)
    if bf16:
        import torch
        Q = torch.from_numpy(Q).bfloat16().float().numpy()
        K = torch.from_numpy(K).bfloat16().float().numpy()
    return Q, K


def row_kind(p: int) -> str:
    return ROW_KINDS[p] if p < len(ROW_KINDS) else "planted"


# ------------------------------------------------------------------------------------------------ the cases
# The smallest shapes that reach each branch; the GPU tests and the CPU mutation checks run the same lists.
_PN = [(1, 1), (1, 257), (63, 2), (63, 255), (64, 1), (64, 256), (64, 513), (65, 257), (65, 2), (130, 255), (130, 256),
       (130, 513)]
_DS = [1, 3, 4, 12, 16, 17, 32, 33, 64, 65, 100, 128]
LSM_F32 = [(P, N, 12) for P, N in _PN] + [(P, N, D) for P, N in ((65, 257), (130, 513)) for D in _DS if D != 12]
SWEEP_P = 9                                                   # one row of every kind and one planted at random
SWEEP = [("f32", N, D) for D in (129, 200, 256) for N in (1, 255, 257, 1025)] + \
        [("bf16", N, D) for D in (12, 16, 100, 128, 129, 256) for N in (1, 255, 257, 1025)]
# (res, m, e); the second block: both sides of the fused pool's LDS limit 3 res (DP + 1) 4 <= 65536
MATRICES = [(res, m, e) for res in (1, 2, 3, 5, 16) for m in (1, 257, 700) for e in (12, 20, 40, 100)]
MATRICES_LIMIT = [(42, 257, 100), (43, 257, 100), (84, 70, 40), (85, 70, 40), (165, 33, 20), (166, 33, 20)]
POOL_ONLY = [(1, 257), (2, 257), (3, 257), (16, 257), (255, 5)]          # (res, m)
# (r, scale, e, m); the second block: both sides of scale^2 res (DP + 1) 4 <= 65536 at e 40, scale 4
PATCH = [(r, s, e, 257 if r < 50 else 70) for r, s in ((6, 1), (7, 2), (50, 3), (7, 4), (18, 4), (50, 5)) for e in (7, 12, 20, 40)]
PATCH_LIMIT = [(60, 4, 40, 70), (64, 4, 40, 70)]
CELLS = [c for c in PATCH if c[1] <= 4]


def fused_pool(res: int, e: int) -> bool:
    DP = 16 if e <= 16 else 32 if e <= 32 else 64 if e <= 64 else 128
    return 3 * res * (DP + 1) * 4 <= 65536


def patch_row_kernel(r: int, scale: int, e: int) -> bool:
    DP = 16 if e <= 16 else 32 if e <= 32 else 64 if e <= 64 else 128
    return e <= 128 and scale * scale * (r // scale) * (DP + 1) * 4 <= 65536


@functools.lru_cache(maxsize=4)
def _inputs_cached(P, N, D, bf16):
    return make_inputs(P, N, D, bf16)


def patch_inputs(r: int, e: int, m: int):
    Q, K = _inputs_cached(r * r, m, e, False)
    return Q.reshape(r, r, e), K


def pool_input(res: int, m: int) -> np.ndarray:
    """A (res^2, m) f32 matrix of distinct negative values (a log-probability matrix's sign)."""
    rng = np.random.default_rng(res * 1000 + m)
    return (-0.1 - np.abs(rng.normal(0, 3, (res * res, m)))).astype(np.float32)
