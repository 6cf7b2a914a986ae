"""tests/corr_matrix_ref.py checked on the host: (1) the f64 reference against the reference project's own expressions
(torch f64, 1e-12); (2) the comparison `|device - ref| <= bound` has teeth: on EVERY case tests/test_gpu_corr_matrices.py
runs, each single-bug restatement of the reference (a row with its neighbour's lse, a key left out of the lse, a shifted or
zero-padded pool window, the wrong centre pixel, trailing pixels, a key taken one index low) falls outside the bound — and
the inputs are scaled so that every bound is at most 1e-3 of its row's spread.

No-ops listed on purpose (the mutation is skipped there): `lse_next_row` at P = 1; `key_prev` at N = 1; both pool
mutations at m = 1 (log_softmax over one key is 0 everywhere) and `pool_shift_x` at res = 1; `centre_low` at odd scales;
`trailing` where r is a multiple of scale.  The spread condition leaves out rows without a spread: N = 1 and the zero query.

Largest bound per case family (max over the family's cases and elements; the +-60 rows set it):
    corr_logsoftmax f32   D = 1: 4.7e-5   3: 6.2e-5   4: 6.9e-5   12: 1.3e-4   16: 1.6e-4   17: 1.7e-4   32: 2.8e-4
                          33: 2.9e-4   64: 5.2e-4   65: 5.3e-4   100: 7.9e-4   128: 9.9e-4
    three-sweep f32       D = 129: 1.0e-3   200: 1.6e-3   256: 2.0e-3
    three-sweep bf16      D = 12: 1.3e-4   16: 1.6e-4   100: 7.9e-4   128: 9.9e-4   129: 1.0e-3   256: 2.0e-3
    corr_matrices         e = 12: 1.3e-4   20: 1.9e-4   40: 3.4e-4   100: 7.9e-4 (fused-limit cases included)
    patch_corr / cells    e = 7: 9.1e-5   12: 1.3e-4   20: 1.9e-4   40: 3.4e-4
(`python -m tests.test_corr_matrix_ref_cpu` prints the table.)  Away from the +-60 rows no bound exceeds 5.4e-4 (D = 256);
the smallest is 8 u = 4.8e-7 (the zero query, N = 1)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import corr_matrix_ref as cr


# ------------------------------------------------------------------ (1) the reference against the reference's expressions
@pytest.mark.parametrize("P,N,D", [(1, 1, 3), (7, 5, 12), (33, 300, 40), (9, 257, 129)])
def test_log_softmax_is_torch_log_softmax(P, N, D):
    Q, K = cr.make_inputs(P, N, D)
    q, k = torch.from_numpy(Q).double(), torch.from_numpy(K).double()
    want = torch.log_softmax(q @ k.T, 1).numpy()
    out, L, lse, w = cr.parts(Q, K)
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lse, torch.logsumexp(q @ k.T, 1).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(w, torch.softmax(q @ k.T, 1).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(w.sum(1), 1.0, rtol=0, atol=1e-12)


def test_log_softmax_of_bf16_inputs_uses_the_bf16_values():
    Q, K = cr.make_inputs(9, 40, 16, bf16=True)
    qb, kb = torch.from_numpy(Q).bfloat16(), torch.from_numpy(K).bfloat16()
    assert torch.equal(qb.float(), torch.from_numpy(Q)) and torch.equal(kb.float(), torch.from_numpy(K))
    want = torch.log_softmax(qb.double() @ kb.double().T, 1).numpy()
    np.testing.assert_allclose(cr.log_softmax(qb, kb), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("res,m", [(1, 3), (2, 5), (3, 4), (7, 9)])
def test_pool3_is_max_pool2d(res, m):
    mat = torch.from_numpy(cr.pool_input(res, m)).double()
    want = F.max_pool2d(mat.view(res, res, m).permute(2, 0, 1)[None], kernel_size=3, stride=1, padding=1)[0]
    got = cr.pool3(mat.numpy(), res)
    np.testing.assert_allclose(got, want.permute(1, 2, 0).reshape(res * res, m).numpy(), rtol=0, atol=1e-12)


def _patch_statement(query_img, obj_keys, res, ds):
    """poseEstSurf.py:72-96 as oracle/estimate_pose_oracle.py:corr_matrices_patch writes it, in f64, before the 3 x 3 pool."""
    e, m = query_img.shape[-1], obj_keys.shape[0]
    R = res * ds
    q = query_img[:R, :R]
    off = ds // 2
    full = torch.log_softmax(q.reshape(R * R, e) @ obj_keys.T, dim=1).view(R, R, m)
    centre = full[off::ds, off::ds].reshape(res * res, m)
    blk = F.max_pool2d(full.permute(2, 0, 1), ds)
    return centre, blk.permute(1, 2, 0).reshape(res * res, m)


@pytest.mark.parametrize("r,scale,e,m", [(6, 1, 7, 9), (7, 2, 12, 20), (11, 3, 12, 17), (7, 4, 20, 5), (18, 4, 5, 6), (11, 5, 3, 4)])
def test_patch_is_the_per_pixel_statement(r, scale, e, m):
    qi, K = cr.patch_inputs(r, e, m)
    c_want, b_want = _patch_statement(torch.from_numpy(qi).double(), torch.from_numpy(K).double(), r // scale, scale)
    centre, bmax, cb, bb = cr.patch(qi, K, scale)
    np.testing.assert_allclose(centre, c_want.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(bmax, b_want.numpy(), rtol=0, atol=1e-12)
    assert (bb >= cb).all() and (bmax >= centre).all()


def test_bound_is_the_stated_formula():
    Q, K = cr.make_inputs(9, 40, 12)
    out, L, lse, w = cr.parts(Q, K)
    b = cr.bound(Q, K, lse, w)
    u, g = 2.0 ** -24, 13 * 2.0 ** -24
    for p, n in [(0, 0), (3, 39), (4, 7), (8, 20)]:
        S = np.abs(Q[p].astype(np.float64) * K.astype(np.float64)).sum(1)
        want = g * S[n] + g * (w[p] * S).sum() + 8 * u * max(1.0, abs(lse[p]), abs(L[p, n]))
        assert abs(b[p, n] - want) <= 1e-15
    assert np.allclose(out[2], -np.log(40.0), rtol=0, atol=1e-12)        # the zero query: -log N everywhere
    assert (np.abs(L[3] - 60.0) < 5.0).all() and (np.abs(L[4] + 60.0) < 5.0).all()
    assert np.signbit(Q[7, 1::3]).all() and (Q[7, 1::3] == 0).all()


# ------------------------------------------------------------------ (2) teeth, on every GPU case
# the docstring's table: the largest bound any case of descriptor width D may have
STATED = {1: 4.7e-5, 3: 6.2e-5, 4: 6.9e-5, 7: 9.1e-5, 12: 1.3e-4, 16: 1.6e-4, 17: 1.7e-4, 20: 1.9e-4, 32: 2.8e-4, 33: 2.9e-4,
          40: 3.4e-4, 64: 5.2e-4, 65: 5.3e-4, 100: 7.9e-4, 128: 9.9e-4, 129: 1.0e-3, 200: 1.6e-3, 256: 2.0e-3}


def _spread_ok(out, bnd):
    spread = out.max(1) - out.min(1)
    rows = spread > 0
    return bool((bnd.max(1)[rows] <= 1e-3 * spread[rows]).all())


def _check_matrix_case(P, N, D, bf16=False, slack=0.0):
    Q, K = cr.make_inputs(P, N, D, bf16)
    ref, bnd = cr.matrix(Q, K)
    assert cr.compare(ref, ref, bnd) and (bnd > 0).all()
    assert _spread_ok(ref, bnd), "a bound above 1e-3 of its row's spread"
    assert bnd.max() <= STATED[D]
    muts = [m for m in cr.LSM_MUTATIONS if not (m == "lse_next_row" and P == 1) and not (m == "key_prev" and N == 1)]
    for mut in muts:
        assert not cr.compare(cr.matrix(Q, K, mut)[0], ref, bnd + slack), mut
    return float(bnd.max())


@pytest.mark.parametrize("P,N,D", cr.LSM_F32)
def test_mutations_fail_corr_logsoftmax_f32(P, N, D):
    _check_matrix_case(P, N, D)


@pytest.mark.parametrize("kind,N,D", cr.SWEEP)
def test_mutations_fail_three_sweep(kind, N, D):
    _check_matrix_case(cr.SWEEP_P, N, D, bf16=(kind == "bf16"), slack=cr.SWEEP_CAP)     # even with the largest constant allowed


def _check_matrices_case(res, m, e):
    Q, K = cr.make_inputs(res * res, m, e)
    ref, bnd = cr.matrix(Q, K)
    pooled, pb = cr.pool3(ref, res), cr.pool3(bnd, res)
    assert _spread_ok(ref, bnd) and bnd.max() <= STATED[e]
    for mut in cr.LSM_MUTATIONS:
        if (mut == "lse_next_row" and res == 1) or (mut == "key_prev" and m == 1):
            continue
        bad = cr.matrix(Q, K, mut)[0]
        assert not cr.compare(bad, ref, bnd), mut
        assert not cr.compare(cr.pool3(bad, res), pooled, pb), mut
    for mut in cr.POOL_MUTATIONS:
        if m == 1 or (mut == "pool_shift_x" and res == 1):
            continue
        assert not cr.compare(cr.pool3(ref, res, mut), pooled, pb), mut
    return float(bnd.max())


@pytest.mark.parametrize("res,m,e", cr.MATRICES + cr.MATRICES_LIMIT)
def test_mutations_fail_corr_matrices(res, m, e):
    _check_matrices_case(res, m, e)


@pytest.mark.parametrize("res,m", cr.POOL_ONLY)
def test_mutations_fail_pool_only(res, m):
    raw = cr.pool_input(res, m).astype(np.float64)
    want = cr.pool3(raw, res)
    for mut in cr.POOL_MUTATIONS:
        if mut == "pool_shift_x" and res == 1:
            continue
        assert not cr.compare(cr.pool3(raw, res, mut), want, 0.0), mut


def _check_patch_case(r, scale, e, m):
    qi, K = cr.patch_inputs(r, e, m)
    centre, bmax, cb, bb = cr.patch(qi, K, scale)
    res = r // scale
    R = res * scale
    full, fb = cr.matrix(qi[:R, :R].reshape(R * R, e), K)
    assert _spread_ok(full, fb) and fb.max() <= STATED[e]
    slack = cr.SWEEP_CAP if scale <= 4 else 0.0       # the cells kernel runs these cases under the three-sweep rule
    pooled, pb = cr.pool3(bmax, res), cr.pool3(bb, res)
    muts = list(cr.LSM_MUTATIONS)
    if scale % 2 == 0:
        muts.append("centre_low")
    if r % scale:
        muts.append("trailing")
    for mut in muts:
        c2, b2, _, _ = cr.patch(qi, K, scale, mut)
        assert not (cr.compare(c2, centre, cb + slack) and cr.compare(b2, bmax, bb + slack)), mut
    for mut in cr.POOL_MUTATIONS:
        if mut == "pool_shift_x" and res == 1:
            continue
        assert not cr.compare(cr.pool3(bmax, res, mut), pooled, pb + slack), mut
    return float(max(cb.max(), bb.max()))


@pytest.mark.parametrize("r,scale,e,m", cr.PATCH + cr.PATCH_LIMIT)
def test_mutations_fail_patch_corr(r, scale, e, m):
    _check_patch_case(r, scale, e, m)


def test_case_lists_sit_on_both_sides_of_every_limit():
    assert [cr.fused_pool(res, e) for res, m, e in cr.MATRICES_LIMIT] == [True, False] * 3
    assert all(cr.fused_pool(res, e) for res, m, e in cr.MATRICES)
    assert cr.fused_pool(321, 12) and not cr.fused_pool(322, 12) and 322 * 322 > 65535
    assert [cr.patch_row_kernel(r, s, e) for r, s, e, m in cr.PATCH_LIMIT] == [True, False]
    assert all(cr.patch_row_kernel(r, s, e) for r, s, e, m in cr.PATCH)
    assert not cr.patch_row_kernel(64, 4, 100) and not cr.patch_row_kernel(55, 5, 40)
    assert all(a * b <= 3_000_000 for a, b in [(P, N) for P, N, D in cr.LSM_F32] + [(r * r, m) for r, m, e in cr.MATRICES + cr.MATRICES_LIMIT]
               + [(r * r, m) for r, s, e, m in cr.PATCH + cr.PATCH_LIMIT] + [(r * r, m) for r, m in cr.POOL_ONLY])
    assert {D for _, _, D in cr.LSM_F32} == {1, 3, 4, 12, 16, 17, 32, 33, 64, 65, 100, 128}


if __name__ == "__main__":
    fam = {}
    for P, N, D in cr.LSM_F32:
        fam[("lsm f32", D)] = max(fam.get(("lsm f32", D), 0), _check_matrix_case(P, N, D))
    for kind, N, D in cr.SWEEP:
        fam[("sweep " + kind, D)] = max(fam.get(("sweep " + kind, D), 0), _check_matrix_case(cr.SWEEP_P, N, D, kind == "bf16", cr.SWEEP_CAP))
    for res, m, e in cr.MATRICES + cr.MATRICES_LIMIT:
        fam[("matrices", e)] = max(fam.get(("matrices", e), 0), _check_matrices_case(res, m, e))
    for c in cr.PATCH + cr.PATCH_LIMIT:
        fam[("patch", c[2])] = max(fam.get(("patch", c[2]), 0), _check_patch_case(*c))
    for k, v in sorted(fam.items()):
        print(k, f"{v:.2e}")
