"""CPU: the key field's arithmetic as host code (csrc/field_mlp.hpp through isr_field_eval_host / isr_field_sin_host): sin32
within 1 ulp of the true sine on |a| <= 2^17, NaN for non-finite input; the host evaluation against an f64 evaluation of the
same weights, inside a margin measured from a plain torch f32 forward; argument errors without a device; the ctypes table
against include/isr_field.h."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import KeyField
from tests import field_ref

ROOT = Path(__file__).resolve().parent.parent
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _sin32(hip_lib, a):
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    assert hip_lib.isr_field_sin_host(vp(a), a.size, vp(out)) == 0
    return out


def test_sin32_within_one_ulp(hip_lib):
    rng = np.random.default_rng(0)
    lim = 2.0 ** 17
    n = 600_000
    logs = np.exp(rng.uniform(np.log(1e-38), np.log(lim), n)) * rng.choice([-1.0, 1.0], n)
    halfpi = np.arange(-83443, 83444) * (np.pi / 2)                 # every multiple of pi/2 inside the range
    a = np.concatenate([rng.uniform(-lim, lim, n), np.linspace(-lim, lim, 100_001), logs, halfpi,
                        [0.0, lim, -lim, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754942e-38]]).astype(np.float32)
    a = a[np.abs(a) <= lim]
    assert a.size >= 10 ** 6
    got = _sin32(hip_lib, a).astype(np.float64)
    ref = np.sin(a.astype(np.float64))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(got - ref) / ulp
    print("sin32: max error", err.max(), "ulp at", a[np.argmax(err)])
    assert err.max() <= 1.0
    assert np.all(np.abs(got) <= 1.0)
    z = _sin32(hip_lib, np.array([0.0, -0.0], np.float32))
    assert z[0] == 0 and z[1] == 0 and not np.signbit(z[0]) and np.signbit(z[1])


def test_sin32_non_finite_and_far_inputs(hip_lib):
    assert np.isnan(_sin32(hip_lib, np.array([np.nan, np.inf, -np.inf], np.float32))).all()
    far = np.array([2.0 ** 18, -2.0 ** 40, 3e38, -3.4e38, 1e20], np.float32)
    got = _sin32(hip_lib, far)
    assert np.all(np.abs(got) <= 1.0) and np.array_equal(got, _sin32(hip_lib, far))


@pytest.mark.parametrize("last", ["sine", "linear"])
def test_host_eval_inside_the_measured_margin(hip_lib, last):
    """3 -> 64 -> 64 -> 12, omega 30.  E_ref: the largest error of a plain torch f32 forward of the same layers against the
    f64 evaluation; the host build may be off by 2 E_ref (the factor covers a different summation order)."""
    widths = (3, 64, 64, 12)
    omegas = (30.0, 30.0, 30.0 if last == "sine" else None)
    Ws, bs = field_ref.siren_params(widths, omegas, seed=1)
    pts = np.random.default_rng(2).uniform(-1, 1, (4096, 3)).astype(np.float32)
    ref = field_ref.eval_f64(Ws, bs, omegas, pts)
    e_ref = float(np.abs(field_ref.TorchField(Ws, bs, omegas)(torch.from_numpy(pts)).numpy().astype(np.float64) - ref).max())
    got = KeyField(Ws, bs, omegas, None).eval_host(pts)
    e_host = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"last={last}: host build {e_host:.3e}, torch f32 forward {e_ref:.3e}")
    field_ref.record("cpu", {f"3-64-64-12 omega 30 last {last}": {"E_ref_torch_f32": e_ref, "E_host_build": e_host}})
    assert e_ref > 0 and e_host <= 2 * e_ref


def test_host_eval_is_the_written_chain(hip_lib):
    """The pack round trip and the definition: fmaf chain from the bias, k ascending, one f32 multiply by omega (narrow
    row-major layers and matrix-core-ordered layers, padded widths)."""
    widths = (3, 5, 40, 33, 7)
    omegas = (30.0, 1.5, None, 2.0)
    Ws, bs = field_ref.siren_params(widths, omegas, seed=3)
    pts = np.random.default_rng(4).uniform(-1, 1, (9, 3)).astype(np.float32)
    got = KeyField(Ws, bs, omegas, None).eval_host(pts)
    want = np.empty_like(got)
    for n in range(len(pts)):
        h = pts[n].astype(np.float64)
        for W, b, om in zip(Ws, bs, omegas):
            z = b.astype(np.float64)
            for k in range(W.shape[1]):            # an f32 fmaf: the f64 product and sum are exact enough to round once
                z = (W[:, k].astype(np.float64) * h[k] + z).astype(np.float32).astype(np.float64)
            if om is not None:
                z = _sin32(hip_lib, (np.float32(om) * z.astype(np.float32))).astype(np.float64)
            h = z
        want[n] = h
    assert np.array_equal(got, want)


def test_argument_errors_without_a_device(hip_lib):
    L = hip_lib
    w = np.array([3, 64, 12], np.int32)
    nb = L.isr_field_pack_bytes(2, vp(w))
    assert nb > 0 and nb % 4 == 0
    bad = [(0, w), (9, np.array([3] + [8] * 9, np.int32)), (2, np.array([4, 64, 12], np.int32)),
           (2, np.array([3, 257, 12], np.int32)), (2, np.array([3, 64, 33], np.int32)), (2, np.array([3, 0, 12], np.int32))]
    for n, ww in bad:
        assert L.isr_field_pack_bytes(n, vp(ww)) == 0 and L.isr_last_error()
    assert L.isr_field_pack_bytes(2, None) == 0
    W = np.zeros(64 * 3 + 12 * 64, np.float32)
    b = np.zeros(76, np.float32)
    om = np.ones(2, np.float32)
    sn = np.ones(2, np.int32)
    pack = np.zeros(nb // 4, np.float32)
    assert L.isr_field_pack(2, vp(w), vp(W), vp(b), vp(om), vp(sn), vp(pack), nb) == 0
    assert L.isr_field_pack(2, vp(w), None, vp(b), vp(om), vp(sn), vp(pack), nb) == -1 and b"null" in L.isr_last_error()
    assert L.isr_field_pack(2, vp(w), vp(W), vp(b), vp(om), vp(sn), None, nb) == -1
    assert L.isr_field_pack(2, vp(w), vp(W), vp(b), vp(om), vp(sn), vp(pack), nb - 4) == -1 and b"pack_bytes" in L.isr_last_error()
    assert L.isr_field_pack(2, vp(np.array([3, 300, 12], np.int32)), vp(W), vp(b), vp(om), vp(sn), vp(pack), nb) == -1
    pts = np.zeros((4, 3), np.float32)
    out = np.zeros((4, 12), np.float32)
    for fn, tail in ((L.isr_field_eval, (None,)), (L.isr_field_eval_host, ())):      # refused before any device is touched
        assert fn(None, nb, 2, vp(w), vp(pts), 4, vp(out), 12, *tail) == -1
        assert fn(vp(pack), nb, 2, None, vp(pts), 4, vp(out), 12, *tail) == -1
        assert fn(vp(pack), nb, 2, vp(w), None, 4, vp(out), 12, *tail) == -1
        assert fn(vp(pack), nb, 2, vp(w), vp(pts), 4, None, 12, *tail) == -1
        assert fn(vp(pack), nb, 2, vp(w), vp(pts), 4, vp(out), 11, *tail) == -1 and b"ld_out" in L.isr_last_error()
        assert fn(vp(pack), nb, 2, vp(w), vp(pts), -1, vp(out), 12, *tail) == -1
        assert fn(vp(pack), nb + 4, 2, vp(w), vp(pts), 4, vp(out), 12, *tail) == -1
        assert fn(vp(pack), nb, 9, vp(w), vp(pts), 4, vp(out), 12, *tail) == -1
        assert fn(vp(pack), nb, 2, vp(w), None, 0, None, 12, *tail) == 0              # N = 0: valid, nothing to do
    assert L.isr_field_sin_host(None, 3, vp(out)) == -1 and L.isr_field_sin_host(None, 0, None) == 0


def test_key_field_refuses_cpu_tensors_and_bad_shapes(hip_lib):
    Ws, bs = field_ref.siren_params((3, 8, 4), (30.0, None))
    f = KeyField(Ws, bs, (30.0, None), None)
    assert f.widths == (3, 8, 4) and f.out_features == 4
    with pytest.raises(_capi.IsrError):
        f(torch.zeros(5, 3))
    with pytest.raises(_capi.IsrError):
        KeyField(Ws, bs, (30.0, None), "cpu")
    with pytest.raises(ValueError):
        KeyField(Ws, bs[:1], (30.0, None), None)
    with pytest.raises(ValueError):
        KeyField([Ws[0], Ws[1][:, :5]], bs, (30.0, None), None)
    with pytest.raises(_capi.IsrError):
        KeyField([np.zeros((40, 3), np.float32)], [np.zeros(40, np.float32)], (None,), None)     # last width > 32
    lin = [torch.nn.Linear(3, 8), torch.nn.Linear(8, 4)]
    with pytest.raises(_capi.IsrError):                      # modules on the CPU: their device is no GPU
        KeyField.from_linears(lin, (30.0, None))
    g = KeyField([m.weight for m in lin], [m.bias for m in lin], (30.0, None), None)
    assert g.eval_host(np.zeros((2, 3), np.float32)).shape == (2, 4)
    import imagesequenceregistrationfor6dposeestimationlabeling_amd as pkg
    assert pkg.KeyField is KeyField


def test_field_signatures_match_the_header(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_field.h").read_text(), flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(isr_field_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(decls) == sorted(_capi.FIELD_SIGNATURES) and len(decls) == 5
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_field.h but not exported"
        assert len(_capi.FIELD_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    assert not set(_capi.FIELD_SIGNATURES) & set(_capi.SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_hip.h").read_text(), flags=re.S)
    assert "isr_field_" not in main
