"""CPU: the host build of csrc/resample.hpp (isr_sample_pdf_host, isr_resample_lengths_host) against the NumPy restatement of
include/isr_resample.h, bit for bit; properties that need no tolerance; and the torch restatement of pytorch3d's
sample_pdf_python (from memory: the rule is UNPINNED) in f64, fed the host's own units.

The parity bound is not a measurement.  A sample is excused only by a rule decided from the f64 restatement alone
(tests/resample_ref.excused_f64): its bin's cdf step lies within 2^-20 of eps, or its unit lies within 2^-20 of a knot that
borders such a bin — there the reference's own `den < eps` test is on a knife edge and f32 torch itself jumps by up to a
whole bin.  With random units at most 0.5 % of the samples may be excused; every other sample may deviate from the f64
restatement by at most 4 x the f32 torch restatement's own largest deviation from it on the same inputs, the project's
margin for f32-against-f64 parity.  With det units the same deviation bound holds, but u_0 = 0 and u_{n-1} = 1 sit exactly on
the end knots by construction, which border an empty (knife-edge) bin on every ray whose weights sum to about 1: their share
is 2 / n of those rays whatever the arithmetic, and is recorded, not capped.  Figures: profiles/resample_parity.json
(python -m tests.resample_ref)."""
import json

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
from tests import resample_ref as rf
from tests.resample_ref import ROOT

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _rows(rng, N, P, kind="random"):
    ln = np.sort(rng.uniform(0.1, 3.0, (N, P)).astype(f32), axis=1)
    w = (rng.uniform(0, 1, (N, P)).astype(f32) ** 6)
    if kind == "zero":
        w[:] = 0
    elif kind == "spike":
        w[:] = 0
        w[np.arange(N), rng.integers(1, P - 1, N)] = 1
    elif kind == "heavy":
        w *= f32(1e4)
    elif kind == "repeated":
        ln[:, 1:] = np.where(rng.uniform(size=(N, P - 1)) < 0.5, ln[:, :-1], ln[:, 1:])
        ln = np.sort(ln, axis=1)
    elif kind == "unsorted":
        ln = rng.permuted(ln, axis=1)
    return np.ascontiguousarray(ln), np.ascontiguousarray(w)


@pytest.mark.parametrize("P", [3, 4, 5, 64, 257])
def test_host_equals_restatement(hip_lib, P):
    rng = np.random.default_rng(P)
    for n in (1, 7, P, 2 * P):
        for add in (False, True):
            for det in (False, True):
                ln, w = _rows(rng, 3, P)
                got = ops.resample_lengths_host(ln, w, n, add, det, seed=77)
                assert same(got, rf.resample_lengths_np(ln, w, n, add, det, seed=77)), (P, n, add, det)


@pytest.mark.parametrize("kind", ["zero", "spike", "heavy", "repeated", "unsorted"])
def test_host_equals_restatement_on_degenerate_rows(hip_lib, kind):
    rng = np.random.default_rng(5)
    for P, n in ((5, 7), (64, 64)):
        for det in (False, True):
            ln, w = _rows(rng, 4, P, kind)
            got = ops.resample_lengths_host(ln, w, n, True, det, seed=3)
            assert same(got, rf.resample_lengths_np(ln, w, n, True, det, seed=3)), (kind, P, det)
            bins, wi = rf.mid_points(ln), np.ascontiguousarray(w[:, 1:-1])
            z = ops.sample_pdf_host(bins, wi, n, det, seed=3)
            want = np.stack([rf.sample_pdf_np(bins[i], wi[i], rf.units(n, det, 3, i)) for i in range(4)])
            assert same(z, want), (kind, P, det)


def test_det_with_one_sample_and_large_seed(hip_lib):
    ln, w = _rows(np.random.default_rng(1), 2, 9)
    assert same(ops.resample_lengths_host(ln, w, 1, False, True), rf.resample_lengths_np(ln, w, 1, False, True))
    seed = (0xDEADBEEF << 32) | 0x12345678
    assert same(ops.resample_lengths_host(ln, w, 5, True, False, seed=seed), rf.resample_lengths_np(ln, w, 5, True, False, seed=seed))


def test_ray_ids_make_a_row_independent_of_its_batch(hip_lib):
    ln, w = _rows(np.random.default_rng(2), 200, 16)         # 200 rows: the host's threaded path
    ids = np.arange(200, dtype=np.int32)[::-1] * 3 + 5
    full = ops.resample_lengths_host(ln, w, 16, True, False, seed=4, ray_ids=ids)
    assert same(full, rf.resample_lengths_np(ln, w, 16, True, False, seed=4, ray_ids=ids))
    for i in (0, 77, 199):
        alone = ops.resample_lengths_host(ln[i:i + 1], w[i:i + 1], 16, True, False, seed=4, ray_ids=ids[i:i + 1])
        assert same(alone[0], full[i])
    default = ops.resample_lengths_host(ln, w, 16, True, False, seed=4)
    assert same(default, ops.resample_lengths_host(ln, w, 16, True, False, seed=4, ray_ids=np.arange(200, dtype=np.int32)))
    assert not same(default, full)


def test_nan_weight_row(hip_lib):
    ln, w = _rows(np.random.default_rng(3), 3, 12)
    clean = ops.resample_lengths_host(ln, w, 6, True, False, seed=1)
    w2 = w.copy()
    w2[1, 4] = np.nan
    out = ops.resample_lengths_host(ln, w2, 6, True, False, seed=1)
    assert same(out[[0, 2]], clean[[0, 2]])
    assert same(out[1, :12], ln[1]) and (bits(out[1, 12:]) == 0x7FC00000).all()      # NaN samples, sorted last
    assert same(out, rf.resample_lengths_np(ln, w2, 6, True, False, seed=1))
    w2[1, 0] = w2[1, 11] = np.nan                                                    # the end weights are not read
    w2[1, 4] = w[1, 4]
    assert same(ops.resample_lengths_host(ln, w2, 6, True, False, seed=1), clean)


def test_properties(hip_lib):
    rng = np.random.default_rng(4)
    for P, n in ((5, 9), (33, 33), (64, 200)):
        for det in (False, True):
            ln, w = _rows(rng, 6, P)
            bins, wi = rf.mid_points(ln), np.ascontiguousarray(w[:, 1:-1])
            z = ops.sample_pdf_host(bins, wi, n, det, seed=8)
            assert (z >= bins[:, :1]).all() and (z <= bins[:, -1:]).all()            # every sample lies in [bins_0, bins_nb]
            if det:
                assert (np.diff(z, axis=1) >= 0).all()                               # det samples do not decrease
            for add in (False, True):
                out = ops.resample_lengths_host(ln, w, n, add, det, seed=8)
                assert out.shape == (6, n + (P if add else 0)) and (np.diff(out, axis=1) >= 0).all()
                assert same(np.sort(out, axis=1), np.sort(np.concatenate([ln, z], axis=1) if add else z, axis=1))
                if add:
                    for i in range(6):
                        assert np.isin(bits(ln[i]), bits(out[i])).all()              # every input length, bit for bit


def test_spike_draws_nearly_every_sample_from_its_bin(hip_lib):
    eps = 1e-5
    for P, n, j in ((10, 64, 3), (64, 256, 40), (257, 100, 0), (257, 1024, 254)):
        nb = P - 2
        bins = np.ascontiguousarray(np.linspace(0.5, 2.5, nb + 1, dtype=f32)[None])
        w = np.zeros((1, nb), f32)
        w[0, j] = 1
        z = ops.sample_pdf_host(bins, w, n, True, eps)[0]
        inside = int(((z >= bins[0, j]) & (z <= bins[0, j + 1])).sum())
        assert inside >= int(np.floor(n * (1 - nb * eps))) - 2, (P, n, j, inside)


@pytest.mark.parametrize("P", rf.PARITY_P)
def test_parity_with_the_torch_restatement(hip_lib, P):
    random, det = rf.parity(P, det=False), rf.parity(P, det=True)
    print(json.dumps([random, det]))
    recorded = {(c["P"], c["det"]): c for c in json.loads((ROOT / "profiles" / "resample_parity.json").read_text())["cases"]}
    assert (P, False) in recorded and (P, True) in recorded
    assert random["excused_share"] <= rf.MAX_EXCUSED
    for case in (random, det):
        assert case["torch_f32_max_dev_kept"] > 0
        assert case["host_max_dev_kept"] <= rf.PARITY_MARGIN * case["torch_f32_max_dev_kept"], case


def test_refusals(hip_lib):
    ln, w = _rows(np.random.default_rng(6), 2, 8)
    ok = dict(n_samples=4)
    with pytest.raises(ValueError):
        ops.resample_lengths_host(ln[:, :2], w[:, :2], **ok)                         # P < 3
    with pytest.raises(ValueError):
        ops.resample_lengths_host(ln, w, 0)                                          # n < 1
    with pytest.raises(ValueError):
        ops.resample_lengths_host(ln, w, 1025)
    with pytest.raises(ValueError):
        ops.resample_lengths_host(np.zeros((1, 1025), f32), np.zeros((1, 1025), f32), 4)
    for eps in (0.0, -1e-5, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            ops.resample_lengths_host(ln, w, 4, eps=eps)
    with pytest.raises(ValueError):
        ops.resample_lengths_host(ln, w[:, :7], 4)                                   # mismatched shapes
    with pytest.raises(ValueError):
        ops.resample_lengths_host(ln, w[:1], 4)
    with pytest.raises(ValueError):
        ops.resample_lengths_host(ln, w, 4, ray_ids=np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        ops.resample_lengths_host(ln.astype(np.float64), w, 4)
    with pytest.raises(ValueError):
        ops.sample_pdf_host(ln, w, 4)                                                # bins need one more column than weights
    with pytest.raises(ValueError):
        ops.sample_pdf_host(ln[:, :1], w[:, :0], 4)                                  # nb < 1
    with pytest.raises(ValueError):
        ops.resample_lengths_host(ln, w, 4, seed=-1)
    with pytest.raises(_capi.IsrError):
        ops.resample_lengths(torch.from_numpy(ln), torch.from_numpy(w), 4)           # no CPU fallback
    with pytest.raises(_capi.IsrError):
        ops.sample_pdf(torch.from_numpy(ln), torch.from_numpy(w[:, :7]), 4)


def test_c_entries_refuse_what_the_header_says(hip_lib):
    import ctypes
    L = hip_lib
    a = np.zeros((1, 8), f32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((1, 16), f32)
    for N, P, n, eps in ((1, 2, 4, 1e-5), (1, 1025, 4, 1e-5), (1, 8, 0, 1e-5), (1, 8, 1025, 1e-5), (1, 8, 4, 0.0),
                         (1, 8, 4, float("inf")), (-1, 8, 4, 1e-5), (2 ** 28 + 1, 8, 4, 1e-5)):
        assert L.isr_resample_lengths_host(p(a), p(a), N, P, n, 1, 1, eps, 0, None, p(out)) < 0, (N, P, n, eps)
        assert L.isr_resample_lengths(p(a), p(a), N, P, n, 1, 1, eps, 0, None, p(out), None) < 0, (N, P, n, eps)
        assert L.isr_last_error()
    assert L.isr_sample_pdf_host(p(a), p(a), 1, 0, 4, 1, 1e-5, 0, None, p(out)) < 0
    assert L.isr_sample_pdf_host(p(a), p(a), 1, 1023, 4, 1, 1e-5, 0, None, p(out)) < 0
    assert L.isr_resample_lengths_host(None, p(a), 1, 8, 4, 1, 1, 1e-5, 0, None, p(out)) < 0
    assert L.isr_resample_lengths_host(None, None, 0, 8, 4, 1, 1, 1e-5, 0, None, None) == 0       # no rays: nothing to do


def test_signature_table_matches_the_header():
    import re
    text = (ROOT / "include" / "isr_resample.h").read_text()
    body = text[text.index("#ifndef ISR_RESAMPLE_H"):]
    names = set(re.findall(r"^int (isr_[a-z_]+)\(", body, re.M))
    assert names == set(_capi.RESAMPLE_SIGNATURES)
    for name, (_, args) in _capi.RESAMPLE_SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, body).group(1)
        assert len(args) == len(decl.split(",")), name
