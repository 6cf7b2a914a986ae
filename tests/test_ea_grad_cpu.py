"""CPU: the host build of csrc/ea_grad.hpp (isr_ea_march_backward_host) against the NumPy restatement of include/isr_ea_grad.h
(tests/ea_grad_ref.py), bit for bit; its weights chain against isr_ea_march_host's; against the reference's executed marcher
under torch autograd (tests/golden/ref_ea_grad.npz) within 4 times the reference-f32's own deviation from its f64;
losses.huber against the reference's executed function; and the refusals of the C entries."""
import ctypes
import json
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, losses, ops

from . import ea_grad_ref as ref

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
CASES = ref.cases()


def vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host(case, need=(True, True)):
    rho, feat, dimage, dw, thr = case
    return ops.ea_march_backward_host(rho, feat, dimage, dw, thr, need)


@pytest.mark.parametrize("name", list(CASES))
def test_host_equals_the_restatement(hip_lib, name):
    rho, feat, dimage, dw, thr = CASES[name]
    dd, df = host(CASES[name])
    want_dd, want_df, want_w = ref.backward_ref(rho, feat, dimage, dw, thr)
    assert ref.same_bits(dd, want_dd) and ref.same_bits(df, want_df)
    assert ref.same_bits(want_w, ops.ea_march_host(rho, feat, thr)[1])                # the chain is the forward's own
    only_dd, none = host(CASES[name], (True, False))                                  # each output left out
    assert none is None and ref.same_bits(only_dd, dd)
    none, only_df = host(CASES[name], (False, True))
    assert none is None and ref.same_bits(only_df, df)


@pytest.mark.parametrize("name", list(CASES))
def test_dfeatures_is_the_forward_weight_times_dimage(hip_lib, name):
    rho, feat, dimage, dw, thr = CASES[name]
    w = ops.ea_march_host(rho, feat, thr)[1]
    with np.errstate(invalid="ignore", over="ignore"):
        assert ref.same_bits(host(CASES[name])[1], w[:, :, None] * dimage[:, None, :-1])


def test_a_nan_ray_leaves_the_clean_rays_alone(hip_lib):
    rho, feat, dimage, dw, thr = CASES["one NaN ray among clean rays"]
    dd, df = host((rho, feat, dimage, dw, thr))
    assert np.isnan(dd[3]).any() and np.isnan(df[3]).any()
    for r in (0, 1, 2, 4, 5):
        solo_dd, solo_df = host((rho[r:r + 1], feat[r:r + 1], dimage[r:r + 1], dw[r:r + 1], thr))
        assert np.isfinite(dd[r]).all() and ref.same_bits(dd[r:r + 1], solo_dd) and ref.same_bits(df[r:r + 1], solo_df)
    # before the NaN sample the ray's weights are clean, so dfeatures is.  ddensities takes the NaN from the adjoint in front
    # of the sample and from T_k behind it; at the sample itself T_11 * (g_11 - a_12) does not read c_11
    assert np.isfinite(df[3, :11]).all() and np.isnan(df[3, 11:]).all()
    assert np.isnan(dd[3, :11]).all() and np.isfinite(dd[3, 11]) and np.isnan(dd[3, 12:]).all()


def test_non_finite_dimage_and_features_stay_in_their_rays(hip_lib):
    for name, row in (("dimage with a NaN", 2), ("dimage with an infinity", 4)):
        dd, df = host(CASES[name])
        clean = [r for r in range(6) if r != row]
        assert np.isfinite(dd[clean]).all() and np.isfinite(df[clean]).all() and not np.isfinite(dd[row]).all()
    df = host(CASES["dimage with a NaN"])[1]                                          # channel 1 of ray 2, and nowhere else
    assert np.isnan(df[2, :, 1]).all() and np.isfinite(df[2][:, [0, 2]]).all()
    assert np.isfinite(host(CASES["dimage with an infinity"])[1]).all()               # the opacity's: no feature reads it
    dd, df = host(CASES["features with a NaN and an infinity"])
    assert np.isfinite(df).all() and np.isfinite(dd[[0, 2, 3, 5]]).all()              # dfeatures does not read the features
    assert np.isnan(dd[1, :6]).all() and np.isfinite(dd[1, 6:]).all()                 # the adjoint runs down from sample 5


def test_null_dweights_equals_zeros(hip_lib):
    a, b = host(CASES["dweights null"]), host(CASES["dweights of zeros"])
    assert ref.same_bits(a[0], b[0]) and ref.same_bits(a[1], b[1])


def test_zero_dimage_signs(hip_lib):
    dd, df = host(CASES["dimage of -0"])
    rho = CASES["dimage of -0"][0]
    assert (np.signbit(df) == (rho > 0)[:, :, None]).all() and not df.any()           # w_k * -0
    dd0, df0 = host((*CASES["dimage of zeros"][:3], None, -1.0))
    assert not dd0.any() and not df0.view(np.uint32).any()


def test_threshold_mode(hip_lib):
    for t in (0.02, 0.0, 2.0):
        rho, feat, dimage, dw, thr = CASES[f"threshold mode, {t}"]
        dd, df = host((rho, feat, dimage, dw, thr))
        assert not dd.view(np.uint32).any()                                           # +0 everywhere, the NaN ray included
        w = ops.ea_march_host(rho, feat, thr)[1]
        assert set(np.unique(w)) <= {0.0, 1.0} and (w.sum(1) <= 1).all()               # binary: the first sample above
        assert ref.same_bits(df, w[:, :, None] * dimage[:, None, :-1])
    assert not host(CASES["threshold mode, 2.0"])[1].any()                            # nothing above 2: no weight at all


def test_densities_of_one_need_no_special_path(hip_lib):
    """Where torch's cumprod backward leaves its division for another route, the recurrence is an ordinary input: against
    the expression in f64 (whose eps keeps 1 - c away from 0) within the bound of the fixture's worse shape."""
    for name in ("densities all 1", "an exact 1 mid-ray", "densities all 0"):
        rho, feat, dimage, dw, thr = CASES[name]
        d = torch.from_numpy(rho).double().requires_grad_(True)
        f = torch.from_numpy(feat).double().requires_grad_(True)
        image, w = ref.pren_march(d, f)
        ((image * torch.from_numpy(dimage).double()).sum() + (w * torch.from_numpy(dw).double()).sum()).backward()
        dd, df = host(CASES[name])
        assert np.isfinite(dd).all() and np.isfinite(df).all()
        E = max(ref.fixture(t)["E_dd"] for t in ref.FIXTURES)
        assert np.abs(dd - d.grad.numpy()).max() <= ref.bound(E, d.grad.numpy())
        assert np.abs(df - f.grad.numpy()).max() <= ref.bound(max(ref.fixture(t)["E_df"] for t in ref.FIXTURES), f.grad.numpy())


def test_against_the_reference_under_autograd(hip_lib):
    """Each gradient array within 4 x the reference-f32's own largest deviation from its f64 (floor: one f32 ulp of the array's
    largest magnitude); no element is excused.  The measured ratios go to profiles/ea_grad_parity.json when ISR_RECORD_PARITY is set."""
    record = {}
    for tag in ref.FIXTURES:
        fx = ref.fixture(tag)
        dd, df = ops.ea_march_backward_host(fx["rho"], fx["feat"], fx["Wi"], fx["Ww"])
        for name, got, want, E in (("ddensities", dd, fx["dd64"], fx["E_dd"]), ("dfeatures", df, fx["df64"], fx["E_df"])):
            err = float(np.abs(got.astype(np.float64) - want).max())
            record[f"{tag}_{name}"] = {"shape": list(got.shape), "E_ref": E, "err": err, "err_over_E_ref": err / E,
                                       "bound": ref.bound(E, want)}
            print(f"{tag} {name}: err {err:.3e} = {err / E:.2f} x E_ref {E:.3e}; bound {ref.bound(E, want):.3e}")
            assert err <= ref.bound(E, want)
    if os.environ.get("ISR_RECORD_PARITY"):                                          # tests do not write unless asked to
        ref.PARITY.write_text(json.dumps(record, indent=1, sort_keys=True) + "\n")


def test_fixture_is_what_its_generator_promises(hip_lib):
    for tag, shape in (("train", (40, 64, 3)), ("wide", (40, 256, 12))):
        fx = ref.fixture(tag)
        assert fx["feat"].shape == shape and fx["rho"].min() >= 0 and fx["rho"].max() <= 1 - 2.0 ** -10 and fx["Ww"].any()
        assert 0 < fx["E_dd"] and 0 < fx["E_df"]


def test_huber_against_the_reference(hip_lib):
    z = np.load(ref.GOLDEN)
    x, y = torch.from_numpy(z["huber_x"]), torch.from_numpy(z["huber_y"])
    for s, tag in ((0.1, "default"), (0.5, "half")):
        got = losses.huber(x, y) if tag == "default" else losses.huber(x, y, scaling=s)
        got64 = losses.huber(x.double(), y.double(), s).numpy()
        assert got.dtype == torch.float32 and got.shape == x.shape
        np.testing.assert_allclose(got64, z[f"huber_{tag}64"], rtol=1e-14, atol=0)
        # f32: seven roundings at the magnitude of the root, sqrt(1 + d^2 / s^2) (>= 1), times s
        tol = 8 * 2.0 ** -24 * s * np.sqrt(1 + (z["huber_x"].astype(np.float64) - z["huber_y"]) ** 2 / s ** 2)
        assert (np.abs(got.numpy() - z[f"huber_{tag}32"]) <= tol).all() and (np.abs(got.numpy() - got64) <= tol).all()
        assert not got.numpy()[0].any()                                               # x = y: exactly 0
    xg = x.clone().requires_grad_(True)
    losses.huber(xg, y).abs().mean().backward()
    assert torch.isfinite(xg.grad).all() and not xg.grad[0].any() and xg.grad[1:].abs().sum() > 0


def test_refusals_and_no_rays(hip_lib):
    L = hip_lib
    rho, feat, dimage, dw = np.zeros((2, 5), f32), np.zeros((2, 5, 3), f32), np.zeros((2, 4), f32), np.zeros((2, 5), f32)
    dd, df = np.full((2, 5), 7, f32), np.full((2, 5, 3), 7, f32)
    dev = lambda *a: L.isr_ea_march_backward(*a, None)
    for entry in (L.isr_ea_march_backward_host, dev):
        for hole in (0, 1, 6):
            a = [vp(rho), vp(feat), 2, 5, 3, -1.0, vp(dimage), vp(dw), vp(dd), vp(df)]
            a[hole] = None
            assert entry(*a) == -1 and b"null" in L.isr_last_error()
        for N, P, F, thr, word in ((-1, 5, 3, -1.0, b"N < 0"), (2, 0, 3, -1.0, b"P outside"), (2, 4097, 3, -1.0, b"P outside"),
                                   (2, 5, 0, -1.0, b"F outside"), (2, 5, 65, -1.0, b"F outside"), (2, 5, 3, float("nan"), b"NaN")):
            assert entry(vp(rho), vp(feat), N, P, F, thr, vp(dimage), vp(dw), vp(dd), vp(df)) == -1 and word in L.isr_last_error()
        assert entry(vp(rho), vp(feat), 2, 5, 3, -1.0, vp(dimage), vp(dw), None, None) == -1 and b"both outputs" in L.isr_last_error()
        assert entry(None, None, 0, 5, 3, -1.0, None, None, vp(dd), vp(df)) == 0      # N = 0: succeeds and touches nothing
        assert entry(vp(rho), vp(feat), 0, 5, 3, 0.5, vp(dimage), vp(dw), vp(dd), None) == 0
        assert entry(None, None, 0, 5, 3, -1.0, None, None, None, None) == 0          # an empty tensor's address is null
        assert entry(None, None, 0, 0, 3, -1.0, None, None, vp(dd), vp(df)) == -1     # the sizes are still checked
    assert (dd == 7).all() and (df == 7).all()
    assert L.isr_ea_march_backward_host(vp(rho), vp(feat), 2, 5, 3, -1.0, vp(dimage), None, vp(dd), None) == 0 and not dd.any()
    assert (df == 7).all()
    empty = ops.ea_march_backward_host(np.zeros((0, 5), f32), np.zeros((0, 5, 3), f32), np.zeros((0, 4), f32))
    assert empty[0].shape == (0, 5) and empty[1].shape == (0, 5, 3)
    for call in (lambda: ops.ea_march_backward_host(rho, feat[:1], dimage), lambda: ops.ea_march_backward_host(rho, feat, dimage[:, :3]),
                 lambda: ops.ea_march_backward_host(rho, feat, dimage, dw[:1]), lambda: ops.ea_march_backward_host(rho, feat, dimage, need=(False, False)),
                 lambda: ops.ea_march_backward_host(rho, feat, dimage, threshold=float("nan"))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_capi.IsrError):
        ops.ea_march_backward(*(torch.from_numpy(a) for a in (rho, feat, dimage)))   # no CPU fall-back


def test_geometry(hip_lib):
    g = ops.ea_grad_geometry()
    assert g == {"threads": 256, "max_group_rays": 64, "row_floats": 4097} and hip_lib.isr_ea_grad_geometry(3) == -1
    for P in range(1, 4097):
        R = ops.ea_grad_rays_per_group(P)
        assert 1 <= R <= g["max_group_rays"] and R * (P | 1) <= max(g["row_floats"], P | 1)
        assert R == g["max_group_rays"] or (R + 1) * (P | 1) > g["row_floats"]
    assert [ops.ea_grad_rays_per_group(P) for P in (1, 64, 128, 256, 4096)] == [64, 63, 31, 15, 1]
    assert hip_lib.isr_ea_grad_rays_per_group(0) == -1 and hip_lib.isr_ea_grad_rays_per_group(4097) == -1


def test_header_and_signature_table(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_ea_grad.h").read_text(), flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(isr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(decls) == sorted(_capi.EA_GRAD_SIGNATURES) and len(decls) == 4
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_ea_grad.h but not exported"
        assert len(_capi.EA_GRAD_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    main = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_hip.h").read_text(), flags=re.S)
    assert "isr_ea_march_backward" not in main and "isr_ea_grad" not in main and hip_lib.isr_abi_version() == 6


def test_the_autograd_route_refuses_cpu_tensors(hip_lib):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import rays
    d, f = torch.zeros((2, 5, 1), requires_grad=True), torch.zeros((2, 5, 3))
    with pytest.raises(_capi.IsrError):
        rays.EmissionAbsorptionRaymarcherStratified()(d, f)
    with pytest.raises(_capi.IsrError):
        rays.EmissionAbsorptionRaymarcherStratified()(d.detach(), f)
