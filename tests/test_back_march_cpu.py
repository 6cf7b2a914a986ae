"""CPU: the march from the far end of the ray (csrc/field_density.hpp's march_ray_back behind isr_density_march_dir_host and
isr_density_march_given_host) against a NumPy restatement bit for bit, against the reference's own statements
(tests/golden/ref_back_march.npz, made by tests/golden/make_ref_back_march.py), and the header / exports / ctypes table."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
from tests import back_march_ref as br
from tests import density_ref as dr

ROOT = Path(__file__).resolve().parent.parent
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
_cache = {}


def _field(H, hidden, n_layers, seed):
    key = (H, hidden, n_layers, seed)
    if key not in _cache:
        Ws, bs = dr.fixture(H, hidden, n_layers, seed)
        _cache[key] = DensityField(Ws, bs, dr.frequencies(H), 10.0, None)
    return _cache[key]


@pytest.mark.parametrize("threshold", [0.2, -1.0])
@pytest.mark.parametrize("P,R", [(1, 5), (2, 5), (33, 130), (128, 5)])
def test_host_back_march_is_the_written_march(hip_lib, P, R, threshold):
    """Negative lengths (the maximum is over the products), a zero length, and direction both = front followed by back."""
    f = _field(4, 32, 1, 3)
    o, d, ln = br.rays(R, P, 100 * P + R)
    ln[1] = -ln[1]
    ln[2, 0] = 0.0
    front = f.march_host(o, d, ln, threshold)
    back = f.march_host(o, d, ln, threshold, direction="back")
    both = f.march_host(o, d, ln, threshold, direction="both")
    rho = front["densities"]
    assert np.array_equal(bits(back["densities"]), bits(rho)) and np.array_equal(bits(both["densities"]), bits(rho))
    wts, depth, hit = br.march_back(ln, rho, threshold)
    assert np.array_equal(bits(back["weights"]), bits(wts))
    assert np.array_equal(bits(back["depth"]), bits(depth))
    assert np.array_equal(back["hit"], hit)
    assert np.array_equal(bits(back["points"]), bits(dr.surface(o, d, depth)))
    assert both["weights"].shape == (R, 2 * P) and both["depth"].shape == (2, R) and both["points"].shape == (2, R, 3)
    assert np.array_equal(bits(both["weights"][:, :P]), bits(front["weights"]))
    assert np.array_equal(bits(both["weights"][:, P:]), bits(back["weights"]))
    for k in ("depth", "points"):
        assert np.array_equal(bits(both[k][0]), bits(front[k])) and np.array_equal(bits(both[k][1]), bits(back[k])), k
    assert np.array_equal(both["hit"][0], front["hit"]) and np.array_equal(both["hit"][1], back["hit"])
    if threshold >= 0:
        assert np.array_equal(front["hit"], back["hit"])
        if P >= 33:
            assert (back["depth"] != front["depth"]).any()          # some ray has a first hit that is not its last


def test_back_march_on_given_densities(hip_lib):
    """By hand: no hit, first and last differ, negative lengths, NaN densities in both modes."""
    nan = np.float32(np.nan)
    ln = np.array([[0.5, 1.0, 1.5], [0.5, 1.0, 1.5], [-0.5, -1.0, -1.5], [-0.5, -1.0, -1.5], [0.5, 1.0, 1.5], [0.5, 1.0, 1.5]],
                  np.float32)
    rho = np.array([[0.1, 0.1, 0.1], [0.9, 0.1, 0.9], [0.9, 0.9, 0.1], [0.0, 0.0, 0.0], [0.9, nan, 0.1], [nan, 0.3, nan]],
                   np.float32)
    wts, depth, hit = ops.density_march_given_host(ln, rho, 0.2, "back")
    assert np.array_equal(wts, [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]])      # a NaN is not above
    assert np.array_equal(hit, [0, 1, 1, 0, 1, 1])
    assert depth[0] == 0 and depth[1] == 1.5 and depth[4] == 0.5 and depth[5] == 1.0
    assert depth[2] == 0 and np.signbit(depth[2]) and depth[3] == 0 and np.signbit(depth[3])      # max(-0, -1, -0): the first stays
    for thr in (0.2, -1.0):
        got = ops.density_march_given_host(ln, rho, thr, "back")
        want = br.march_back(ln, rho, thr)
        for g, w in zip(got[:2], want[:2]):
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(bits(g)[~np.isnan(w)], bits(w)[~np.isnan(w)])
        assert np.array_equal(got[2], want[2])
    soft = ops.density_march_given_host(ln, rho, -1.0, "back")
    assert np.isnan(soft[0][4, :2]).all() and soft[0][4, 2] == np.float32(0.1) and np.isnan(soft[1][4]) and soft[2][4] == 1
    assert np.allclose(soft[0][1], [0.9 * 0.9 * 0.1, 0.1 * 0.1, 0.9], rtol=1e-6)
    both = ops.density_march_given_host(ln, rho, 0.2, "both")
    front = ops.density_march_given_host(ln, rho, 0.2, "front")
    assert np.array_equal(both[0][:, :3], front[0]) and np.array_equal(both[0][:, 3:], wts)
    assert np.array_equal(bits(both[1][0]), bits(front[1])) and np.array_equal(bits(both[1][1]), bits(depth))


def test_against_the_reference_s_statements(hip_lib):
    """prenBack.py:362-385 executed on recorded densities (its thresholdMode compares against the literal 0.05).  Threshold
    mode: equal.  Soft mode: within torch-f32's own deviation from the same march in f64 on those inputs (x 4, the density
    field's convention), recorded in profiles/density_field_parity.json."""
    g = np.load(ROOT / "tests" / "golden" / "ref_back_march.npz")
    rho, ln = g["rho"][0], g["lengths"][0]
    P = rho.shape[1]
    wts, depth, hit = ops.density_march_given_host(ln, rho, 0.05, "both")
    assert np.array_equal(wts, g["threshold_weights"][0])
    assert np.array_equal(depth[0], g["threshold_depth_front"][0]) and np.array_equal(depth[1], g["threshold_depth_back"][0])
    back = wts[:, P:]
    assert not back[0].any() and back[1, -1] == 1 and back[2, -1] == 1 and back[3, 0] == 1 and not back[4].any()
    assert np.array_equal(hit[1], (g["threshold_weights"][0][:, P:] != 0).any(axis=1))

    wts, depth, _ = ops.density_march_given_host(ln, rho, -1.0, "back")
    ref_w, ref_d = g["soft_weights"][0][:, P:], g["soft_depth_back"][0]
    w32, d32 = br.torch_march_back(torch.from_numpy(rho), torch.from_numpy(ln), -1.0)
    assert np.array_equal(w32.numpy(), ref_w) and np.array_equal(d32.numpy(), ref_d)      # the restatement is the reference's
    w64, d64 = br.torch_march_back(torch.from_numpy(rho).double(), torch.from_numpy(ln).double(), -1.0)
    e_ref_w = float(np.abs(ref_w.astype(np.float64) - w64.numpy()).max())
    e_ref_d = float(np.abs(ref_d.astype(np.float64) - d64.numpy()).max())
    e_w = float(np.abs(wts.astype(np.float64) - w64.numpy()).max())
    e_d = float(np.abs(depth.astype(np.float64) - d64.numpy()).max())
    e_vs_ref = float(np.abs(wts - ref_w).max())
    print(f"soft back march: weights host {e_w:.3e} torch f32 {e_ref_w:.3e} (host - reference {e_vs_ref:.3e}); "
          f"depth host {e_d:.3e} torch f32 {e_ref_d:.3e}")
    dr.record("cpu soft back march", {f"recorded densities, {rho.shape[0]} rays x {P}": {
        "E_ref_torch_f32_weights": e_ref_w, "E_host_build_weights": e_w, "E_ref_torch_f32_depth": e_ref_d,
        "E_host_build_depth": e_d, "host_minus_reference_weights": e_vs_ref}})
    assert e_ref_w > 0 and e_w <= 4 * e_ref_w and e_d <= 4 * e_ref_d


def test_refusals_and_signatures(hip_lib):
    L = hip_lib
    vp = lambda a: a.ctypes.data_as(_capi.C.c_void_p)
    f = _field(4, 32, 1, 3)
    o, d, ln = br.rays(4, 2, 1)
    dep, pts, hit = np.zeros(8, np.float32), np.zeros((8, 3), np.float32), np.zeros(8, np.int32)
    w = np.array([32], np.int32)
    for fn, tail in ((L.isr_density_march_dir, (None,)), (L.isr_density_march_dir_host, ())):      # refused before any device is touched
        call = lambda P=2, way=1, thr=0.2, N=4: fn(vp(f.pack_host), f.pack_host.nbytes, 1, vp(w), 4, vp(o), vp(d), vp(ln), N, P, thr,
                                                   way, None, None, vp(dep), vp(pts), vp(hit), *tail)
        assert call(way=3) == -1 and b"direction" in L.isr_last_error()
        assert call(way=-1) == -1
        assert call(thr=float("nan")) == -1 and b"NaN" in L.isr_last_error()
        assert call(P=0) == -1 and call(P=4097) == -1
        assert call(N=0) == 0
    assert L.isr_density_march_dir_host(vp(f.pack_host), f.pack_host.nbytes, 1, vp(w), 4, vp(o), vp(d), vp(ln), 4, 2, 0.2, 2, None,
                                        None, vp(dep), vp(pts), vp(hit)) == 0
    with pytest.raises(ValueError):
        f.march_host(o, d, ln, 0.2, direction="sideways")
    with pytest.raises(ValueError):
        ops.density_march_given_host(ln, ln[:, :1], 0.2)
    for header, table, n in (("isr_density_dir.h", _capi.DENSITY_DIR_SIGNATURES, 3), ("isr_radius.h", _capi.RADIUS_SIGNATURES, 3)):
        text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
        decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(isr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
        assert sorted(decls) == sorted(table) and len(decls) == n
        for name, params in decls.items():
            assert hasattr(hip_lib, name), f"{name} declared in {header} but not exported"
            assert len(table[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    others = (_capi.SIGNATURES, _capi.FIELD_SIGNATURES, _capi.FPS_SIGNATURES, _capi.DENSITY_SIGNATURES, _capi.MC_SIGNATURES)
    assert not any((set(_capi.DENSITY_DIR_SIGNATURES) | set(_capi.RADIUS_SIGNATURES)) & set(o) for o in others)
    main = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_hip.h").read_text(), flags=re.S)
    assert "isr_radius_" not in main and "march_dir" not in main
