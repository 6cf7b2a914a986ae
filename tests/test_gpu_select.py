"""GPU parity: ops.select_top / ops.gather_corr (isr_select_top_batch / isr_gather_corr_batch at B = 1) vs the literal reference expressions
(inference.py:274-290) evaluated with torch on the CPU — integer-exact given identical values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref_filter(in1):
    """inference.py:282-288 verbatim semantics on a (P,1) tensor."""
    if len(in1) > 500:
        perc = int(0.8 * len(in1))
        threshval = torch.sort(in1[:, 0])[0][-perc + 1]
    else:
        threshval = torch.sort(in1[:, 0])[0][-len(in1) + 1]
    return torch.where(in1[:, 0] > threshval)[0], threshval


@pytest.mark.parametrize("P,kind", [
    (1, "normal"), (2, "normal"), (7, "normal"), (500, "normal"), (501, "normal"), (5625, "normal"),
    (307200, "normal"), (4096, "ties"), (10000, "neg0"), (100001, "wide"),
])
def test_select_top_matches_reference(cuda0, P, kind):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    g = torch.Generator().manual_seed(P)
    x = -torch.rand(P, generator=g) * 10
    if kind == "ties":
        x = torch.round(x)                     # heavy ties around the threshold
    if kind == "neg0":
        x[::3] = -0.0
        x[1::3] = 0.0
    if kind == "wide":
        x = torch.randn(P, generator=g) * 1e20   # positive and negative, huge range
    if P == 1:
        ref_idx, ref_thr = torch.where(x > x[0])[0], x[0]     # [-1 + 1] = index 0
    else:
        ref_idx, ref_thr = _ref_filter(x[:, None])
    keep, M, thr = ops.select_top(x.to(cuda0))
    torch.cuda.synchronize()
    m = int(M.item())
    assert float(thr.item()) == float(ref_thr) or (thr.item() == 0 and ref_thr == 0)
    assert m == len(ref_idx)
    assert torch.equal(keep[:m].cpu().long(), ref_idx)


def test_gather_corr(cuda0):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    g = torch.Generator().manual_seed(3)
    P, N = 5000, 800
    idx = torch.randint(N, (P,), generator=g, dtype=torch.int32)
    logp = -torch.rand(P, generator=g)
    pts = torch.randn(N, 3, generator=g)
    pix = torch.rand(P, 2, generator=g) * 75
    keep, M, _ = ops.select_top(logp.to(cuda0))
    p3d, p2d = ops.gather_corr(idx.to(cuda0), keep, M, pts.to(cuda0), pix.to(cuda0))
    torch.cuda.synchronize()
    m = int(M.item())
    nidx = keep[:m].cpu().long()
    assert torch.equal(p3d[:m].cpu(), pts[idx.long()][nidx])     # ep3d = surfacePointsScaled[idx1][nidx]
    assert torch.equal(p2d[:m].cpu(), pix[nidx])


# ------------------------------------------------------------------------------------------------------------------
# Scan spills, chunk edges, the rank rule, value edges and the batched entries against the reference expressions.
def _ref_filter_p(in1, frac, min_n):
    """_ref_filter with 0.8 and 500 replaced by the parameters; raises IndexError where Python does."""
    if len(in1) > min_n:
        perc = int(frac * len(in1))
        threshval = torch.sort(in1[:, 0])[0][-perc + 1]
    else:
        threshval = torch.sort(in1[:, 0])[0][-len(in1) + 1]
    return torch.where(in1[:, 0] > threshval)[0], threshval


def _same_cut(keep, M, thr, ref_idx, ref_thr, what=None):
    m = int(M.item())
    assert float(thr.item()) == float(ref_thr), what
    assert m == len(ref_idx), what
    assert torch.equal(keep[:m].cpu().long(), ref_idx), what


@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_select_top_scan_spill(cuda0, kind):
    """P = 2048 * 1024 + 2048 + 5 = 2 099 205 values are 1026 blocks of kChunk = 2048, so scan_blocks_kernel's
    `const int per = (nblocks + 1023) / 1024;` is 2: both `for (int j = 0; j < per; ++j)` loops run twice per thread
    (`b = t * per + j`; threads past 512 own no block) — the suite so far stopped at 150 blocks, per = 1.  About 80 % of
    the values are kept, spread over every block, so every block's offset matters.  Normal values and heavy ties
    (rounded values), against _ref_filter."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    P = 2048 * 1024 + 2048 + 5
    assert (P + 2047) // 2048 == 1026
    g = torch.Generator().manual_seed(11)
    x = torch.randn(P, generator=g) * 3 - 5
    if kind == "ties":
        x = torch.round(x)
    ref_idx, ref_thr = _ref_filter(x[:, None])
    assert 1025 * 2048 < int(ref_idx[-1]) and len(ref_idx) > P // 2
    keep, M, thr = ops.select_top(x.to(cuda0))
    _same_cut(keep, M, thr, ref_idx, ref_thr)


@pytest.mark.parametrize("P", [2047, 2048, 2049, 4097])
def test_select_top_chunk_edges(cuda0, P):
    """One value short of a block of kChunk = 2048, exactly one block, one value into the second block and one into the
    third: `if (i < P)` of hist_kernel, `if (i0 + e < P)` of count_kernel / scatter_kernel at their edges."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    g = torch.Generator().manual_seed(P)
    x = torch.randn(P, generator=g)
    x[P - 1] = 50.0                                  # the last value is always kept
    ref_idx, ref_thr = _ref_filter(x[:, None])
    assert int(ref_idx[-1]) == P - 1
    keep, M, thr = ops.select_top(x.to(cuda0))
    _same_cut(keep, M, thr, ref_idx, ref_thr)


_RANK_CASES = [
    # frac, min_n, n          int(frac * n), the index the reference reads
    (0.5, 10, 100),         # perc = 50 >= 2: sorted[-49]
    (0.3, 0, 3000),         # perc = 900: more than one block
    (0.15, 5, 10),          # perc = 1: sorted[0], every value above the minimum is kept
    (0.0004, 100, 2600),    # perc = 1 again, over two blocks
    (0.05, 5, 10),          # perc = 0: sorted[1]
    (0.0, 0, 2500),         # perc = 0
    (1.0, 5, 100),          # frac = 1: perc = n, sorted[-n + 1] = sorted[1]
    (1.0, 0, 2),            # frac = 1 at n = 2
    (0.8, 64, 64),          # n == min_n: the short-list arm, sorted[1]
    (0.8, 64, 65),          # n == min_n + 1: perc = 52, sorted[14]
    (0.8, 500, 500), (0.8, 500, 501),
]


@pytest.mark.parametrize("frac,min_n,n", _RANK_CASES)
def test_select_top_rank_rule(cuda0, frac, min_n, n):
    """select_rank against the reference expressions with 0.8 and 500 replaced by the parameters, through the host count
    (n = P) and through a device count (n of P = n + 37 capacity values, the padding winning if it were counted):
    `if (perc == 1) return 0;`, `return (perc >= 1) ? n - perc + 1 : 1;` with perc >= 2 and perc = 0, frac = 1, and
    both sides of `if (n > min_n)`."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    g = torch.Generator().manual_seed(1000 * n + min_n)
    x = torch.randn(n + 37, generator=g)
    x[n:] = 1.0e3
    ref_idx, ref_thr = _ref_filter_p(x[:n, None], frac, min_n)
    perc = int(frac * n)
    if n > min_n and perc == 1:
        assert len(ref_idx) == n - 1 and float(ref_thr) == float(x[:n].min())
    if n > min_n and perc == 0:
        assert len(ref_idx) == n - 2
    keep, M, thr = ops.select_top(x[:n].contiguous().to(cuda0), frac, min_n)
    _same_cut(keep, M, thr, ref_idx, ref_thr, "host count")
    keep, M, thr = ops.select_top(x.to(cuda0), frac, min_n, n_dev=torch.tensor([n], dtype=torch.int32, device=cuda0))
    _same_cut(keep, M, thr, ref_idx, ref_thr, "device count")


@pytest.mark.parametrize("frac,min_n,n", [(1.5, 5, 10), (0.5, 0, 1), (0.0, 0, 1)])
def test_select_top_rank_out_of_range(cuda0, frac, min_n, n):
    """Where the reference raises IndexError (perc > n + 1, or index 1 of a single value): with a device count the image
    keeps nothing (M = 0, thr = +inf: init_state_kernel's `if (n <= 0 || rank < 0 || rank >= n)`), without one the call
    is refused on the host (`ISR_REQUIRE(rank >= 0 && rank < P, ...)`), as include/isr_hip.h states."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
    x = torch.randn(n + 5, generator=torch.Generator().manual_seed(n))
    with pytest.raises(IndexError):
        _ref_filter_p(x[:n, None], frac, min_n)
    keep, M, thr = ops.select_top(x.to(cuda0), frac, min_n, n_dev=torch.tensor([n], dtype=torch.int32, device=cuda0))
    assert int(M.item()) == 0 and float(thr.item()) == float("inf")
    with pytest.raises(_capi.IsrError, match="out of range"):
        ops.select_top(x[:n].contiguous().to(cuda0), frac, min_n)


def _value_edge_case(kind):
    g = torch.Generator().manual_seed(5)
    inf = float("inf")
    if kind == "inf_few":                # a few infinities of both signs among 3000 finite values
        x = torch.randn(3000, generator=g)
        x[[3, 1500, 2999]] = -inf
        x[[0, 7, 2048]] = inf
    elif kind == "neg_inf_threshold":    # short list: sorted[1] is the second -inf; everything finite is kept
        x = torch.randn(300, generator=g)
        x[[5, 100, 299]] = -inf
    elif kind == "pos_inf_threshold":    # 600 finite values of 3000: sorted[601] is +inf, nothing is above it
        x = torch.full((3000,), inf)
        x[::5] = torch.randn(600, generator=g)
    elif kind == "all_equal":
        x = torch.full((5000,), -2.5)
    elif kind == "all_equal_short":
        x = torch.full((300,), 7.0)
    elif kind == "two_values":           # 30 % upper value: thr is the lower value, the upper ones are kept
        x = torch.where(torch.rand(5000, generator=g) < 0.3, torch.tensor(-1.0), torch.tensor(-2.0))
    elif kind == "two_values_high":      # 90 % upper value: thr is the upper value, nothing kept
        x = torch.where(torch.rand(5000, generator=g) < 0.9, torch.tensor(-1.0), torch.tensor(-2.0))
    return x


@pytest.mark.parametrize("kind", ["inf_few", "neg_inf_threshold", "pos_inf_threshold", "all_equal", "all_equal_short",
                                  "two_values", "two_values_high"])
def test_select_top_value_edges(cuda0, kind):
    """+-inf through isr::ordered_bits and `x[i0 + e] > thr`; an all-equal input (the threshold is the value, which is
    the maximum: nothing is strictly above it, M = 0); two distinct values on either side of the cut."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    x = _value_edge_case(kind)
    ref_idx, ref_thr = _ref_filter(x[:, None])
    if kind in ("all_equal", "all_equal_short"):
        assert len(ref_idx) == 0 and float(ref_thr) == float(x[0])
    if kind == "neg_inf_threshold":
        assert float(ref_thr) == float("-inf") and len(ref_idx) == len(x) - 3
    if kind == "pos_inf_threshold":
        assert float(ref_thr) == float("inf") and len(ref_idx) == 0
    if kind == "two_values":
        assert float(ref_thr) == -2.0 and 0 < len(ref_idx) < len(x)
    if kind == "two_values_high":
        assert float(ref_thr) == -1.0 and len(ref_idx) == 0
    keep, M, thr = ops.select_top(x.to(cuda0))
    _same_cut(keep, M, thr, ref_idx, ref_thr)


def test_select_top_batch_matches_reference(cuda0):
    """ops.select_top_batch, B = 9 with ragged device counts in ONE call — 0, 1, 2, min_n, min_n + 1, P and counts on and
    next to a block edge — and padding values past each count that would win if they were counted.  Every image equals
    _ref_filter on its own first n_b values (not merely the single call); a count of 0 keeps nothing with thr = +inf
    (include/isr_hip.h).  Two images alone at B = 1 give the same bits: an image does not depend on its group."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    P = 4100
    counts = [0, 1, 2, 500, 501, P, 2048, 2049, 3000]
    B = len(counts)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, P, generator=g) * 2 - 3
    x[6] = torch.round(x[6])                                  # one image with heavy ties
    for b, n in enumerate(counts):
        x[b, n:] = 1.0e3
    xd = x.to(cuda0)
    n_dev = torch.tensor(counts, dtype=torch.int32, device=cuda0)
    keep, M, thr = ops.select_top_batch(xd, n_dev=n_dev)
    for b, n in enumerate(counts):
        if n == 0:
            assert int(M[b].item()) == 0 and float(thr[b].item()) == float("inf")
            continue
        ref_idx, ref_thr = _ref_filter(x[b, :n, None])
        _same_cut(keep[b], M[b], thr[b], ref_idx, ref_thr, (b, n))
    for b in (4, 7):
        k1, M1, t1 = ops.select_top_batch(xd[b:b + 1], n_dev=n_dev[b:b + 1])
        m = int(M1.item())
        assert m == int(M[b].item()) and torch.equal(k1[0, :m], keep[b, :m]) and torch.equal(t1[0], thr[b]), b


@pytest.mark.parametrize("shared", [True, False])
def test_gather_corr_batch_matches_indexing(cuda0, shared):
    """isr_gather_corr_batch against plain indexing, B = 5: pix_xy shared (P, 2) (`shared_pix ? 0 : (int64_t)P * 2` as
    the image stride) and per image (B, P, 2); M in {0, 1, P} and values in between side by side; idx hitting N - 1.
    Rows m < M[b] equal pts[idx[b]][keep[b, :M]] and pix[keep[b, :M]].  The outputs are pre-filled with NaN through the C
    entry, so a row below M[b] that was not written cannot compare equal.  Rows m >= M[b] are not asserted: the header
    defines p3d / p2d for m < M_dev[b] only and promises nothing about the rest."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi
    g = torch.Generator().manual_seed(21 + shared)
    B, P, N = 5, 700, 50                                      # three blocks of gather_kernel's 256 threads, the last ragged
    Ms = [0, 1, P, 300, 257]
    idx = torch.randint(N, (B, P), generator=g, dtype=torch.int32)
    idx[2, P - 1] = N - 1
    idx[1, :] = N - 1
    idx[3, 0] = 0
    pts = torch.randn(N, 3, generator=g)
    pix = torch.rand((P, 2) if shared else (B, P, 2), generator=g) * 75
    keep = torch.zeros(B, P, dtype=torch.int32)
    for b, m in enumerate(Ms):
        keep[b, :m] = torch.sort(torch.randperm(P, generator=g)[:m])[0].int()
    assert int(keep[2, P - 1]) == P - 1 and int(idx[2, keep[2, P - 1]]) == N - 1
    L = _capi.lib()
    d = lambda t: t.contiguous().to(cuda0)
    idx_d, keep_d, pts_d, pix_d, M_d = d(idx), d(keep), d(pts), d(pix), torch.tensor(Ms, dtype=torch.int32, device=cuda0)
    p3d = torch.full((B, P, 3), float("nan"), dtype=torch.float32, device=cuda0)
    p2d = torch.full((B, P, 2), float("nan"), dtype=torch.float32, device=cuda0)
    with torch.cuda.device(cuda0):
        _capi.check(L.isr_gather_corr_batch(idx_d.data_ptr(), keep_d.data_ptr(), M_d.data_ptr(), P, B, pts_d.data_ptr(), N,
                                            pix_d.data_ptr(), int(shared), p3d.data_ptr(), p2d.data_ptr(),
                                            _capi.current_stream(cuda0)), "isr_gather_corr_batch")
    torch.cuda.synchronize()
    for b, m in enumerate(Ms):
        nidx = keep[b, :m].long()
        assert torch.equal(p3d[b, :m].cpu(), pts[idx[b].long()][nidx]), b
        assert torch.equal(p2d[b, :m].cpu(), (pix if shared else pix[b])[nidx]), b


def test_gather_corr_batch_single_point(cuda0):
    """N = 1: every correspondence is the one surface point; M = P beside M = 0 (through ops.gather_corr_batch)."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    g = torch.Generator().manual_seed(2)
    B, P = 2, 300
    pts = torch.randn(1, 3, generator=g)
    pix = torch.rand(B, P, 2, generator=g) * 75
    idx = torch.zeros(B, P, dtype=torch.int32)
    keep = torch.arange(P, dtype=torch.int32).repeat(B, 1)
    M = torch.tensor([P, 0], dtype=torch.int32)
    p3d, p2d = ops.gather_corr_batch(idx.to(cuda0), keep.to(cuda0), M.to(cuda0), pts.to(cuda0), pix.to(cuda0))
    torch.cuda.synchronize()
    assert torch.equal(p3d[0].cpu(), pts.expand(P, 3)) and torch.equal(p2d[0].cpu(), pix[0])
