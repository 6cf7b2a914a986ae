"""CPU: the density field's arithmetic as host code (csrc/field_density.hpp through the _host entries of
include/isr_density.h): sincos32, softplus32 and density32 within 1 ulp of f64; the host evaluation and the host march bit for
bit against the NumPy restatement of tests/density_ref.py; both against torch's own f32 forward and cumprod march inside
margins measured from torch itself; orderings; refusals; the ctypes table against the header."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
from tests import density_ref as dr

ROOT = Path(__file__).resolve().parent.parent
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sincos(hip_lib, a):
    a = np.ascontiguousarray(a, np.float32)
    s, c = np.empty_like(a), np.empty_like(a)
    assert hip_lib.isr_density_sincos_host(vp(a), a.size, vp(s), vp(c)) == 0
    return s, c


def _ulps(got, ref):
    return np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def _field(H, hidden, n_layers, seed=0, **kw):
    Ws, bs = dr.fixture(H, hidden, n_layers, seed, **kw)
    return DensityField(Ws, bs, dr.frequencies(H), 10.0, None), Ws, bs


@pytest.mark.parametrize("case", ["special", "powers", "frequencies", "bit patterns"])
def test_sincos32_within_one_ulp_of_f64(hip_lib, case):
    """numpy's f64 sin / cos reduce exactly at every magnitude (checked against mpmath when the kernel was written: 1.1e-16)."""
    rng = np.random.default_rng(5)
    if case == "special":
        s, c = _sincos(hip_lib, np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 1.1754942e-38], np.float32))
        assert s[0] == 0 and not np.signbit(s[0]) and s[1] == 0 and np.signbit(s[1]) and np.all(c == 1)
        assert np.array_equal(s[2:], np.array([1e-45, -1e-45, 1e-39, 1.1754942e-38], np.float32))
        s, c = _sincos(hip_lib, np.array([np.inf, -np.inf, np.nan], np.float32))
        assert np.isnan(s).all() and np.isnan(c).all()
        far = np.array([2.0 ** 65, -2.0 ** 100, 3.4e38, -3.4e38, 2.0 ** 127], np.float32)      # beyond 2^64: the same rule
        s, c = _sincos(hip_lib, far)
        assert np.all(np.abs(s) <= 1) and np.all(np.abs(c) <= 1)
        a = far
    elif case == "powers":
        p = (2.0 ** np.arange(-149, 65)).astype(np.float32)
        a = np.concatenate([p, -p])
    elif case == "frequencies":
        x = rng.uniform(-1.2, 1.2, 10 ** 4).astype(np.float32)
        a = (x[:, None] * dr.frequencies(60)[None, :]).reshape(-1)
        assert np.abs(a).max() > 1e16
    else:
        a = rng.integers(0, 2 ** 32, 10 ** 5, dtype=np.uint64).astype(np.uint32).view(np.float32)
        a = a[np.isfinite(a) & (np.abs(a) <= 2.0 ** 64)]
    s, c = _sincos(hip_lib, a)
    es, ec = _ulps(s, np.sin(a.astype(np.float64))), _ulps(c, np.cos(a.astype(np.float64)))
    print(f"sincos32 [{case}]: sine {es.max():.4f} ulp at {a[es.argmax()]!r}, cosine {ec.max():.4f} ulp at {a[ec.argmax()]!r}")
    assert es.max() <= 1.0 and ec.max() <= 1.0
    assert np.all(np.abs(s) <= 1) and np.all(np.abs(c) <= 1)
    small = np.abs(a) < 2.0 ** 17                      # below the old limit the sine is sin32's
    if small.any():
        old = np.empty_like(a[small])
        assert hip_lib.isr_field_sin_host(vp(np.ascontiguousarray(a[small])), old.size, vp(old)) == 0
        assert np.array_equal(bits(old), bits(s[small]))


def test_softplus_and_density_within_one_ulp_of_f64(hip_lib):
    """The header states 0.5001 ulp measured and holds both to 1 ulp.  f64 reference: log1p(exp(beta z)) / beta with the exact
    product beta z (z where it exceeds 20), and -expm1(-s)."""
    rng = np.random.default_rng(6)
    z = np.concatenate([rng.uniform(-12, 4, 200_000), rng.normal(size=100_000) * 1e-3, -np.exp(rng.uniform(-40, 4.3, 100_000)),
                        np.exp(rng.uniform(-40, 5, 100_000)), [0.0, -0.0, 2.0, 2.0000002, 1.9999999, 80.0, -80.0, 3e38, -3e38]]
                       ).astype(np.float32)
    for beta in (10.0, 1.0, 0.37):
        sp, de = np.empty_like(z), np.empty_like(z)
        assert hip_lib.isr_density_activations_host(vp(z), z.size, beta, vp(sp), vp(de)) == 0
        b = np.float64(np.float32(beta))
        t = b * z.astype(np.float64)
        with np.errstate(over="ignore"):
            ref = np.where(t > 20.0, z.astype(np.float64), np.log1p(np.exp(np.minimum(t, 20.0))) / b)
        e1 = _ulps(sp, ref)                              # np.spacing of a subnormal f32 (or 0) is 2^-149: absolute there
        s = np.abs(z)
        with np.errstate(over="ignore"):
            refd = -np.expm1(-s.astype(np.float64))
        dd = np.empty_like(z)
        assert hip_lib.isr_density_activations_host(vp(s), s.size, beta, vp(sp), vp(dd)) == 0
        e2 = _ulps(dd, refd)
        print(f"beta {beta}: softplus32 {e1.max():.4f} ulp, density32 {e2.max():.4f} ulp")
        assert e1.max() <= 1.0 and e2.max() <= 1.0
        assert np.array_equal(bits(dr.softplus32(z, beta)), bits(np.where(np.isnan(sp), sp, dr.softplus32(z, beta))))
    sp, de = np.empty(2, np.float32), np.empty(2, np.float32)
    assert hip_lib.isr_density_activations_host(vp(np.array([np.nan, -np.inf], np.float32)), 2, 10.0, vp(sp), vp(de)) == 0
    assert np.isnan(sp[0]) and sp[1] == 0 and np.isnan(de[0])


def test_numpy_restatement_of_the_activations_is_the_host_build(hip_lib):
    z = np.concatenate([np.random.default_rng(7).uniform(-12, 4, 50_000), [0.0, -0.0, 2.0, 80.0, -80.0]]).astype(np.float32)
    sp, de = np.empty_like(z), np.empty_like(z)
    assert hip_lib.isr_density_activations_host(vp(z), z.size, 10.0, vp(sp), vp(de)) == 0
    assert np.array_equal(bits(sp), bits(dr.softplus32(z, 10.0)))
    s = np.abs(z)
    assert hip_lib.isr_density_activations_host(vp(s), s.size, 10.0, vp(sp), vp(de)) == 0
    assert np.array_equal(bits(de), bits(dr.density32(s)))


SHAPES = [(1, 32, 1, 1), (1, 32, 2, 63), (4, 32, 1, 65), (4, 256, 2, 63), (60, 32, 2, 65), (60, 256, 1, 257), (60, 256, 2, 257),
          (1, 256, 1, 257), (4, 32, 2, 257), (60, 32, 1, 1)]


@pytest.mark.parametrize("H,hidden,n_layers,N", SHAPES)
def test_host_eval_is_the_written_chain(hip_lib, H, hidden, n_layers, N):
    f, Ws, bs = _field(H, hidden, n_layers, seed=H + hidden + n_layers)
    pts = np.random.default_rng(N).uniform(-1.2, 1.2, (N, 3)).astype(np.float32)
    got = f.eval_host(pts)
    want = dr.eval_points(Ws, bs, dr.frequencies(H), 10.0, pts, lambda a: _sincos(hip_lib, a))
    assert np.array_equal(bits(got), bits(want))
    if N >= 63:
        share = float((got > 0.2).mean())
        print(f"H {H} hidden {hidden} layers {n_layers}: {share:.2f} of the points above 0.2")
        assert 0.2 <= share <= 0.8


@pytest.mark.parametrize("H,hidden,n_layers", [(60, 256, 2), (4, 32, 1)])
def test_host_eval_inside_the_margin_torch_f32_sets(hip_lib, H, hidden, n_layers):
    """E_ref: the largest deviation of torch's f32 forward of the same layers from an f64 evaluation of the same network on
    the same inputs; the host build may deviate by 4 E_ref (another summation order, softplus(10) amplifying by up to 10 per
    layer).  Both numbers go to profiles/density_field_parity.json."""
    f, Ws, bs = _field(H, hidden, n_layers, seed=11)
    pts = np.random.default_rng(12).uniform(-1.2, 1.2, (2048, 3)).astype(np.float32)
    tm = dr.TorchDensity(Ws, bs, dr.frequencies(H))
    ref = tm(torch.from_numpy(pts), double=True).numpy().reshape(-1)
    e_ref = float(np.abs(tm(torch.from_numpy(pts)).numpy().reshape(-1).astype(np.float64) - ref).max())
    got = f.eval_host(pts)
    e_host = float(np.abs(got.astype(np.float64) - ref).max())
    share = float((got > 0.2).mean())
    print(f"H {H} {hidden} x {n_layers}: host build {e_host:.3e}, torch f32 forward {e_ref:.3e}, share above 0.2 {share:.2f}")
    dr.record("cpu eval", {f"H {H} hidden {hidden} x {n_layers}": {"E_ref_torch_f32": e_ref, "E_host_build": e_host}})
    assert 0.2 <= share <= 0.8
    assert e_ref > 0 and e_host <= 4 * e_ref


def _rays(R, P, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.5, 0.5, (R, 3)).astype(np.float32)
    d = rng.normal(size=(R, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = np.sort(rng.uniform(0.0, 1.5, (R, P)).astype(np.float32), axis=1)
    return o, d, ln


@pytest.mark.parametrize("threshold", [0.2, -1.0])
@pytest.mark.parametrize("R", [1, 5, 130])
@pytest.mark.parametrize("P", [1, 2, 33, 128])
def test_host_march_is_the_written_march(hip_lib, P, R, threshold):
    f, Ws, bs = _field(4, 32, 1, seed=3)
    o, d, ln = _rays(R, P, 100 * P + R)
    if R >= 5:
        ln[1] = -ln[1]                                  # negative lengths: the maximum is over the products
        ln[2, 0] = 0.0
    h = f.march_host(o, d, ln, threshold)
    pts = (o[:, None, :] + d[:, None, :] * ln[:, :, None]).astype(np.float32)
    rho = f.eval_host(pts.reshape(-1, 3)).reshape(R, P)
    assert np.array_equal(bits(h["densities"]), bits(rho))
    wts, depth, hit = dr.march(ln, rho, threshold)
    assert np.array_equal(bits(h["weights"]), bits(wts))
    assert np.array_equal(bits(h["depth"]), bits(depth))
    assert np.array_equal(h["hit"], hit)
    assert np.array_equal(bits(h["points"]), bits(dr.surface(o, d, depth)))


def test_march_edge_rays(hip_lib):
    """A ray with no hit, a ray whose first point hits, negative lengths — on densities chosen by hand through the march of the
    restatement, and on the field through the host entry (the rays are picked from what the field gives)."""
    ln = np.array([[0.5, 1.0, 1.5], [0.5, 1.0, 1.5], [-0.5, -1.0, -1.5], [-0.5, -1.0, -1.5]], np.float32)
    rho = np.array([[0.1, 0.1, 0.1], [0.9, 0.1, 0.9], [0.1, 0.9, 0.9], [0.0, 0.0, 0.0]], np.float32)
    wts, depth, hit = dr.march(ln, rho, 0.2)
    assert np.array_equal(wts, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]]) and np.array_equal(hit, [0, 1, 1, 0])
    assert depth[0] == 0 and depth[1] == 0.5 and depth[3] == 0 and np.signbit(depth[3])
    assert depth[2] == 0 and np.signbit(depth[2])       # max(-0, -1, -0): the first product stays
    wts, depth, hit = dr.march(ln, rho, -1.0)
    assert np.allclose(wts[1], [0.9, 0.01, 0.081]) and depth[1] == np.float32(0.5) * np.float32(0.9)
    f, _, _ = _field(4, 32, 1, seed=3)
    o, d, ln = _rays(400, 16, 9)
    h = f.march_host(o, d, ln, 0.2)
    first = h["weights"][:, 0] == 1
    assert (h["hit"] == 0).any() and first.any() and ((h["hit"] == 1) & ~first).any()
    none = h["hit"] == 0
    assert np.all(h["depth"][none] == 0) and np.array_equal(h["points"][none], o[none]) and np.all(h["weights"][none] == 0)
    assert np.array_equal(h["depth"][first], ln[first, 0])


@pytest.mark.parametrize("threshold", [0.2, -1.0])
def test_host_march_against_the_cumprod_formulation(hip_lib, threshold):
    """pren.py:342-365 restated with torch on torch's own f32 densities.  Threshold mode: equal, rays with a density within 1e-6
    of the threshold (in either evaluation) left out, at most 2 % of them.  Soft mode: inside 4 x the deviation of torch's f32
    route from the same route in f64."""
    H, hidden, nl, R, P = 60, 256, 2, 256, 24
    f, Ws, bs = _field(H, hidden, nl, seed=21)
    o, d, ln = _rays(R, P, 22)
    h = f.march_host(o, d, ln, threshold)
    tm = dr.TorchDensity(Ws, bs, dr.frequencies(H))
    to, td, tl = torch.from_numpy(o), torch.from_numpy(d), torch.from_numpy(ln)
    pts = to[:, None, :] + td[:, None, :] * tl[:, :, None]
    rho32 = tm(pts)[..., 0]
    w32, dep32 = dr.torch_march(rho32, tl, threshold)
    share = float((h["densities"] > 0.2).mean())
    assert 0.2 <= share <= 0.8
    if threshold >= 0:
        near = (np.abs(rho32.numpy() - 0.2) <= 1e-6) | (np.abs(h["densities"] - 0.2) <= 1e-6)
        left_out = near.any(axis=1)
        print(f"threshold mode: {left_out.mean():.4f} of the rays left out, {share:.2f} of the points above the threshold")
        assert left_out.mean() <= 0.02
        keep = ~left_out
        assert np.array_equal(h["weights"][keep], w32.numpy()[keep])
        assert np.array_equal(h["depth"][keep], dep32.numpy()[keep])
        want = (to + td * dep32[:, None]).numpy()
        assert np.array_equal(h["points"][keep], want[keep])
        assert np.array_equal(h["hit"][keep] != 0, (w32.numpy() != 0).any(axis=1)[keep])
    else:
        rho64 = tm(pts, double=True)[..., 0]
        w64, dep64 = dr.torch_march(rho64, tl.double(), threshold)
        e_ref_w = float((w32.double() - w64).abs().max())
        e_ref_d = float((dep32.double() - dep64).abs().max())
        e_w = float(np.abs(h["weights"].astype(np.float64) - w64.numpy()).max())
        e_d = float(np.abs(h["depth"].astype(np.float64) - dep64.numpy()).max())
        print(f"soft mode: weights host {e_w:.3e} torch f32 {e_ref_w:.3e}; depth host {e_d:.3e} torch f32 {e_ref_d:.3e}")
        dr.record("cpu soft march", {f"H {H} hidden {hidden} x {nl}, {R} rays x {P}": {
            "E_ref_torch_f32_weights": e_ref_w, "E_host_build_weights": e_w, "E_ref_torch_f32_depth": e_ref_d,
            "E_host_build_depth": e_d}})
        assert e_ref_w > 0 and e_w <= 4 * e_ref_w and e_d <= 4 * e_ref_d


def test_grid_order_is_the_reference_s_after_its_movedims():
    """nerf.py:683-700: gridCoords[(ix * R + iy) * R + iz] = (t[iz], t[iy], t[ix]); viewed (R, R, R), movedim(0, 2) and
    movedim(1, 0) give out[i, j, k] = value at (t[i], t[j], t[k]) — what DensityField.grid_densities evaluates in ij order."""
    res = 8
    pts = dr.grid_points(res)
    tag = torch.from_numpy(pts[:, 0] * 1.0 + pts[:, 1] * 10.0 + pts[:, 2] * 100.0).view(res, res, res)
    ref = tag.movedim(0, 2).movedim(1, 0)
    t = torch.from_numpy(np.linspace(-1, 1, res).astype(np.float32))
    mine = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), dim=-1)
    assert torch.equal(ref, mine[..., 0] * 1.0 + mine[..., 1] * 10.0 + mine[..., 2] * 100.0)
    assert np.array_equal(np.sort(pts.reshape(-1)), np.sort(mine.reshape(-1).numpy()))


def test_collect_candidates_order_and_drops():
    """genFeat.py:191-198 on a stand-in field: bundle order, ray order, rays whose point stayed at the origin dropped."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import key_export

    class Fake:
        def surface_points(self, origins, directions, lengths, threshold=0.2):
            depth = lengths[..., 0] * (lengths[..., 0] > threshold)
            return origins + directions * depth[..., None], depth, depth != 0

    mk = lambda o, d, l: SimpleNamespace(origins=torch.tensor(o), directions=torch.tensor(d), lengths=torch.tensor(l))
    b1 = mk([[[0., 0, 0], [1, 1, 1], [2, 2, 2]]], [[[1., 0, 0], [0, 1, 0], [0, 0, 1]]], [[[0.5, 9], [0.1, 9], [0.7, 9]]])
    b2 = mk([[[3., 3, 3]]], [[[1., 1, 1]]], [[[1.0, 9]]])
    got = key_export.collect_candidates(Fake(), [b1, b2], threshold=0.2)
    assert torch.equal(got, torch.tensor([[0.5, 0, 0], [2, 2, 2.7], [4, 4, 4]]))
    with pytest.raises(ValueError):
        key_export.collect_candidates(Fake(), [])


def test_refusals_without_a_device(hip_lib):
    L = hip_lib
    w = np.array([32, 32], np.int32)
    nb = L.isr_density_pack_bytes(2, vp(w), 4)
    assert nb > 0 and nb % 4 == 0
    for n, ww, H in [(2, w, 0), (2, w, 65), (2, np.array([32, 257], np.int32), 4), (5, np.array([8] * 5, np.int32), 4),
                     (0, w, 4), (2, np.array([0, 32], np.int32), 4)]:
        assert L.isr_density_pack_bytes(n, vp(ww), H) == 0 and L.isr_last_error()
    assert L.isr_density_pack_bytes(2, None, 4) == 0
    fr = dr.frequencies(4)
    W = np.zeros(32 * 24 + 32 * 32 + 32, np.float32)
    b = np.zeros(65, np.float32)
    pack = np.zeros(nb // 4, np.float32)
    assert L.isr_density_pack(2, vp(w), 4, vp(fr), 10.0, vp(W), vp(b), vp(pack), nb) == 0
    assert L.isr_density_pack(2, vp(w), 4, vp(fr), 10.0, vp(W), vp(b), vp(pack), nb - 4) == -1 and b"pack_bytes" in L.isr_last_error()
    assert L.isr_density_pack(2, vp(w), 4, vp(fr), 10.0, vp(W), vp(b), vp(pack), nb + 4) == -1
    assert L.isr_density_pack(2, vp(w), 4, None, 10.0, vp(W), vp(b), vp(pack), nb) == -1 and b"null" in L.isr_last_error()
    assert L.isr_density_pack(2, vp(w), 4, vp(fr), 0.0, vp(W), vp(b), vp(pack), nb) == -1 and b"beta" in L.isr_last_error()
    assert L.isr_density_pack(2, vp(w), 65, vp(fr), 10.0, vp(W), vp(b), vp(pack), nb) == -1
    pts, out = np.zeros((4, 3), np.float32), np.zeros(4, np.float32)
    for fn, tail in ((L.isr_density_eval, (None,)), (L.isr_density_eval_host, ())):        # refused before any device is touched
        assert fn(None, nb, 2, vp(w), 4, vp(pts), 4, vp(out), *tail) == -1
        assert fn(vp(pack), nb + 4, 2, vp(w), 4, vp(pts), 4, vp(out), *tail) == -1
        assert fn(vp(pack), nb, 2, vp(w), 4, None, 4, vp(out), *tail) == -1
        assert fn(vp(pack), nb, 2, vp(w), 4, vp(pts), -1, vp(out), *tail) == -1
        assert fn(vp(pack), nb, 2, vp(w), 4, None, 0, None, *tail) == 0                     # N = 0: valid, nothing to do
    ln, dep, hit = np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros(4, np.int32)
    for fn, tail in ((L.isr_density_march, (None,)), (L.isr_density_march_host, ())):
        call = lambda P, N=4, o=vp(pts), thr=0.2: fn(vp(pack), nb, 2, vp(w), 4, o, vp(pts), vp(ln), N, P, thr, None, None, vp(dep),
                                                     vp(pts), vp(hit), *tail)
        assert call(0) == -1 and b"P = 0" in L.isr_last_error()
        assert call(4097) == -1
        assert call(2, o=None) == -1
        assert call(2, thr=float("nan")) == -1
        assert call(2, N=0) == 0
    f, _, _ = _field(4, 32, 1)
    with pytest.raises(_capi.IsrError):
        f.customForwardForDensity(torch.zeros(5, 3))
    with pytest.raises(_capi.IsrError):
        DensityField(*dr.fixture(4, 32, 1), dr.frequencies(4), 10.0, "cpu")
    with pytest.raises(ValueError):
        DensityField(*dr.fixture(4, 32, 1), dr.frequencies(5), 10.0, None)
    with pytest.raises(_capi.IsrError):
        DensityField(*dr.fixture(4, 32, 5), dr.frequencies(4), 10.0, None)
    import imagesequenceregistrationfor6dposeestimationlabeling_amd as pkg
    assert pkg.DensityField is DensityField and callable(pkg.collect_candidates)


def test_density_signatures_match_the_header(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_density.h").read_text(), flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(isr_density_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(decls) == sorted(_capi.DENSITY_SIGNATURES) and len(decls) == 8
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_density.h but not exported"
        assert len(_capi.DENSITY_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    main = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_hip.h").read_text(), flags=re.S)
    assert "isr_density_" not in main
