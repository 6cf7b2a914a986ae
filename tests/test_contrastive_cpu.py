"""CPU: the host twins of the contrastive loss (isr_contrastive_forward_host / _backward_host) against the NumPy restatement
of include/isr_contrastive.h (tests/contrastive_ref.py), bit for bit: shapes from one element to sums that cross every block
of the stated orders (64 columns, 64 and 1024 rows, 256 leaves), both kinds of negatives, the value cases (equal logits, a
dominating positive, logits near +-88 and beyond, duplicated negatives, a NaN row between clean rows, an infinity, upstream
gradients 1, -2.5 and 0), a row alone against the same row in a batch, the refusals and the ctypes table."""
import re

import numpy as np
import pytest

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import IsrError
from tests import contrastive_ref as cr
from tests.contrastive_ref import ROOT, f32, same

SHAPES = [(1, 1, 1, 1), (2, 65, 130, 12), (3, 64, 63, 13), (1, 130, 4097, 12), (2, 257, 64, 64), (1, 1030, 64, 12)]
NAMES = ("m", "t", "pos", "rows", "loss")


def _both(q, k, n, scale=1e-3, g=None):
    fwd = ops.contrastive_forward_host(q, k, n, scale)
    want = cr.forward(q, k, n, scale)
    for name, a, b in zip(NAMES, fwd, want):
        assert same(a, b), name
    bwd = ops.contrastive_backward_host(q, k, n, fwd[0], fwd[1], g, scale)
    ref = cr.backward(q, k, n, scale, fwd[0], fwd[1], 1.0 if g is None else g)
    for name, a, b in zip(("dq", "dk", "dn"), bwd, ref):
        assert same(a, b), name
    return fwd, bwd


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,S,M,D", SHAPES)
def test_host_equals_the_restatement(hip_lib, B, S, M, D, shared):
    rng = np.random.default_rng(B * 1000 + S + M + D)
    q, k, n = cr.inputs(rng, B, S, M, D, 1 if shared else B)
    (m, t, pos, rows, loss), (dq, dk, dn) = _both(q, k, n)
    assert np.isfinite(loss) and np.isfinite(dq).all() and np.isfinite(dn).all()
    assert (t >= 0).all() and (rows >= 0).all()


@pytest.mark.parametrize("rows", cr.TREE_EDGES)
def test_loss_host_at_the_level_edges_of_the_ordered_sum(hip_lib, rows):
    """B S = 1, 256, 257, 65 536 and 65 537 leaves: below, at and above one tree of 256 and two levels of trees."""
    q, k, n = cr.tree_edge_inputs(rows)
    fwd = ops.contrastive_forward_host(q, k, n, 1e-3)
    for name, a, b in zip(NAMES, fwd, cr.forward(q, k, n, 1e-3)):
        assert same(a, b), name
    assert np.isfinite(fwd[4]) and fwd[4] > 0


@pytest.mark.parametrize("g", [1.0, -2.5, 0.0])
def test_upstream_gradient(hip_lib, g):
    q, k, n = cr.inputs(np.random.default_rng(5), 2, 9, 70, 12, 2)
    _, (dq, dk, dn) = _both(q, k, n, g=g)
    if g == 0.0:
        assert not dq.any() and not dk.any() and not dn.any()
    m, t = ops.contrastive_forward_host(q, k, n)[:2]
    only = ops.contrastive_backward_host(q, k, n, m, t, g, need=(False, True, False))
    assert only[0] is None and only[2] is None and same(only[1], dk)


def test_equal_logits_and_a_dominating_positive(hip_lib):
    D, M = 12, 130
    q = np.zeros((1, 3, D), f32)
    k, n = np.ones((1, 3, D), f32), np.ones((1, M, D), f32)
    (m, t, pos, rows, loss), _ = _both(q, k, n, scale=1.0)                   # every logit 0: the row loss is log(1 + M)
    assert (m == 0).all() and np.allclose(rows, np.log(1 + M), rtol=2e-7)
    q[:] = 3.0
    k[:] = 3.0
    n[:] = -3.0                                                              # pos = 108, neg = -108: p underflows to 0
    (m, t, pos, rows, loss), (dq, dk, dn) = _both(q, k, n, scale=1.0)
    assert (pos == 108).all() and (t == 0).all() and (rows == 0).all() and loss == 0
    assert not dq.any() and not dk.any() and not dn.any()


@pytest.mark.parametrize("gap", [80.0, 86.9, 87.0, 87.1, 88.0, 88.8, 104.0, 200.0])
def test_logits_near_the_exponential_cut(hip_lib, gap):
    """One logit at 0 and the rest `gap` below it, on either side: exp32 is 0 below -87 by the rule."""
    D, M = 4, 70
    q = np.ones((1, 2, D), f32)
    k = np.zeros((1, 2, D), f32)
    k[0, 0, 0] = -gap                                                        # row 0: the positive is far below
    n = np.zeros((1, M, D), f32)
    n[0, :, 1] = np.where(np.arange(M) % 3 == 0, 0.0, -gap)
    k[0, 1, 0] = 0.0                                                         # row 1: the positive ties the maximum
    (m, t, pos, rows, loss), (dq, dk, dn) = _both(q, k, n, scale=1.0)
    assert (m == 0).all() and np.isfinite(rows).all() and np.isfinite(dq).all()
    assert rows[0, 0] >= f32(gap) and pos[0, 0] == f32(-gap)


def test_duplicated_negatives(hip_lib):
    rng = np.random.default_rng(8)
    q, k, n = cr.inputs(rng, 2, 7, 66, 12, 2)
    n[:, 1::2] = n[:, 0::2]
    _, (dq, dk, dn) = _both(q, k, n)
    assert same(dn[:, 1::2], dn[:, 0::2])


@pytest.mark.parametrize("shared", [False, True])
def test_a_nan_row_between_clean_rows(hip_lib, shared):
    rng = np.random.default_rng(9)
    q, k, n = cr.inputs(rng, 2, 5, 70, 12, 1 if shared else 2)
    clean_f, clean_b = _both(q, k, n)
    q[0, 2, 3] = np.nan
    (m, t, pos, rows, loss), (dq, dk, dn) = _both(q, k, n)
    nan = np.array([0x7FC00000], np.uint32)
    for a in (m, t, pos, rows, dq, dk):
        assert (a[0, 2].view(np.uint32) == nan).all()
    keep = np.ones((2, 5), bool)
    keep[0, 2] = False
    for a, c in zip((m, t, pos, rows, dq, dk), (*clean_f[:4], *clean_b[:2])):
        assert same(a[keep], c[keep])
    assert loss.view(np.uint32) == nan
    if shared:
        assert (dn.view(np.uint32) == nan).all()
    else:
        assert (dn[0].view(np.uint32) == nan).all() and same(dn[1], clean_b[2][1])


def test_an_infinity(hip_lib):
    rng = np.random.default_rng(10)
    q, k, n = cr.inputs(rng, 1, 4, 66, 12, 1)
    n[0, 5, 0] = -np.inf                                                     # rows with q_0 > 0: one logit -Inf, p = 0
    q[0, :, 0] = np.abs(q[0, :, 0]) + 0.1
    (m, t, pos, rows, loss), (dq, dk, dn) = _both(q, k, n)
    assert np.isfinite(rows).all() and np.isfinite(loss)
    n[0, 5, 0] = np.inf                                                      # +Inf logit: the row is NaN
    (m, t, pos, rows, loss), _ = _both(q, k, n)
    assert np.isinf(m).all() and np.isnan(t).all() and np.isnan(rows).all() and np.isnan(loss)


def test_a_row_alone_and_in_a_batch(hip_lib):
    rng = np.random.default_rng(11)
    q, k, n = cr.inputs(rng, 3, 70, 130, 12, 3)
    full_f = ops.contrastive_forward_host(q, k, n)
    for b, s in ((0, 0), (1, 64), (2, 69)):
        one = ops.contrastive_forward_host(q[b:b + 1, s:s + 1], k[b:b + 1, s:s + 1], n[b:b + 1])
        for a, c in zip(one[:4], full_f[:4]):
            assert same(a[0, 0], c[b, s])
        # dq / c and dk / c of a row do not depend on its batch either: compare at the same c (g cancels the row count)
        dq, dk, _ = ops.contrastive_backward_host(q, k, n, full_f[0], full_f[1], 210.0, need=(True, True, False))
        dq1, dk1, _ = ops.contrastive_backward_host(q[b:b + 1, s:s + 1], k[b:b + 1, s:s + 1], n[b:b + 1], one[0], one[1], 1.0,
                                                    need=(True, True, False))
        assert same(dq1[0, 0], dq[b, s]) and same(dk1[0, 0], dk[b, s])


def test_refusals(hip_lib):
    q, k, n = cr.inputs(np.random.default_rng(0), 2, 3, 4, 5, 2)
    with pytest.raises(IsrError, match="D outside"):
        ops.contrastive_forward_host(*cr.inputs(np.random.default_rng(0), 1, 2, 3, 65, 1))
    with pytest.raises(IsrError, match="Bn must be"):
        ops.contrastive_forward_host(q, k, np.concatenate([n, n[:1]]))
    with pytest.raises(IsrError, match="M outside"):
        ops.contrastive_forward_host(q, k, n[:, :0])
    with pytest.raises(IsrError, match="at least 1"):
        ops.contrastive_forward_host(q[:, :0], k[:, :0], n)
    with pytest.raises(ValueError):
        ops.contrastive_forward_host(q, k[:, :2], n)
    with pytest.raises(ValueError):
        ops.contrastive_forward_host(q.astype(np.float64), k, n)
    L = hip_lib
    assert L.isr_contrastive_workspace_bytes(1 << 14, (1 << 14) + 1, 4, 5, 1) == 0 and b"2^28" in L.isr_last_error()
    assert L.isr_contrastive_workspace_bytes(2, 3, (1 << 24) + 1, 5, 2) == 0
    assert L.isr_contrastive_workspace_bytes(1 << 14, 1 << 14, 1 << 24, 64, 1) > 0
    # a device entry refuses before it touches anything: null pointers never reached
    assert L.isr_contrastive_forward(None, None, None, 2, 3, 4, 0, 2, 1.0, None, None, None, None, None, None, 0, None) == -1
    assert L.isr_contrastive_backward(None, None, None, 2, 3, 4, 5, 3, 1.0, None, None, None, None, None, None, None, 0, None) == -1
    assert L.isr_contrastive_forward(None, None, None, 2, 3, 4, 5, 2, 1.0, None, None, None, None, None, None, 0, None) == -1
    assert b"null pointer" in L.isr_last_error()


def test_geometry_and_splits(hip_lib):
    g = ops.contrastive_geometry()
    assert g == {"group": 64, "tile": 64, "range_rows": 1024, "reduce": 256}
    assert ops.contrastive_column_splits(3, 1030, 65, 12, 1) == 4            # 3090 rows: four ranges
    assert ops.contrastive_column_splits(3, 1030, 65, 12, 3) == 1            # per-item negatives are never split
    assert ops.contrastive_column_splits(1, 1024, 65, 12, 1) == 1            # one range
    assert ops.contrastive_column_splits(16, 1024, 80000, 12, 1) == 1        # enough columns to fill the chip
    assert ops.contrastive_column_splits(16, 1024, 1024, 12, 1) == 16


def test_ctypes_table_matches_the_header(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_contrastive.h").read_text(), flags=re.S)
    decls = dict(re.findall(r"\b(isr_\w+)\s*\(([^)]*)\)\s*;", text))
    assert sorted(decls) == sorted(_capi.CONTRASTIVE_SIGNATURES) and len(decls) == 7
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_contrastive.h but not exported"
        assert len(_capi.CONTRASTIVE_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    main = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_hip.h").read_text(), flags=re.S)
    assert "isr_contrastive" not in main and _capi.ABI_VERSION == 6


def test_package_exports():
    import imagesequenceregistrationfor6dposeestimationlabeling_amd as pkg
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import losses
    import torch
    for name in ("contrastive_loss", "returnCrossEntropy", "returnCrossEntropy2", "returnCrossEntropyWithNeg"):
        assert getattr(pkg, name) is getattr(losses, name)
    x = torch.zeros((1, 2, 3))
    with pytest.raises(IsrError, match="no CPU fallback"):
        losses.contrastive_loss(x, x, x)
