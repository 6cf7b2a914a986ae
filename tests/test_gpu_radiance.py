"""GPU: isr_radiance_render and isr_ea_march against the host build of the same header (bit for bit): per-point densities
and colours, the render at every tiling of rays and points, the early exit against the full route, the fused image against
the march alone, the density entries' outputs, row independence, non-finite rays, outputs written whatever the buffers held,
workspaces and streams, refusals, and the renderer end to end on an 8 x 8 grid."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops, rays, render
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField, FeatureField, KeyField, RadianceField
from tests import density_ref as dr
from tests import poison
from tests import radiance_ref as rr

pytestmark = pytest.mark.gpu
f32 = np.float32
KEYS = ("image", "depth", "points", "hit", "weights", "densities", "colours")
_cache = {}


def _field(net, dev):
    if net not in _cache:
        _cache[net] = rr.device_field(net, dev)
    return _cache[net]


def _dev(f, o, d, ln, thr, weights=True, densities=True, colours=True, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(f.device)
    out = ops.radiance_render(f.rpack, f.widths, f.H, f.Wc, f.C, t(o), t(d), t(ln), threshold=thr, want_weights=weights,
                              want_densities=densities, want_colours=colours, **kw)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _same(got, want, keys=KEYS):
    for k in keys:
        if got[k] is not None and want[k] is not None:
            assert rr.same(got[k], want[k]), k


@pytest.mark.parametrize("N", [1, 63, 65, 130])
@pytest.mark.parametrize("net", rr.NETS)
def test_points_equal_the_host_build(cuda0, net, N):
    """P = 1: a tile holds 64 rays, each with its own direction term; N = 130 is three workgroups, the last one short."""
    f = _field(net, cuda0)
    o, d, ln = rr.bundle(N, 1)
    want = rr.host_field(net)[0].render_host(o, d, ln, -1.0)
    got = _dev(f, o, d, ln, -1.0)
    _same(got, want, ("densities", "colours"))
    b = SimpleNamespace(origins=torch.from_numpy(o).to(cuda0), directions=torch.from_numpy(d).to(cuda0),
                        lengths=torch.from_numpy(ln).to(cuda0))
    dens, col = f.batched_forward(b)
    assert dens.shape == (N, 1, 1) and col.shape == (N, 1, net[4])
    assert rr.same(dens.cpu().numpy().reshape(N, 1), want["densities"]) and rr.same(col.cpu().numpy(), want["colours"])


@pytest.mark.parametrize("threshold", [0.2, -1.0])
@pytest.mark.parametrize("P,N", [(1, 130), (2, 5), (33, 5), (33, 130), (64, 3), (65, 3), (100, 3), (128, 1), (128, 5)])
def test_render_equals_render_host(cuda0, P, N, threshold):
    """Wc = 40: widths that are no multiple of 32.  Ray 1 has a zero direction, every ray its own."""
    net = rr.NETS[1]
    f = _field(net, cuda0)
    o, d, ln = rr.bundle(N, P)
    want = rr.host_field(net)[0].render_host(o, d, ln, threshold)
    _same(_dev(f, o, d, ln, threshold), want)
    _same(_dev(f, o, d, ln, threshold, densities=False, colours=False), want)      # threshold mode, P >= 64: the early exit
    if N > 1:
        assert want["hit"].any() and np.isfinite(want["image"]).all()


@pytest.mark.parametrize("net", [rr.NETS[0], rr.NETS[2]])
def test_early_exit_equals_the_full_route(cuda0, net):
    """Threshold mode, one ray per workgroup: with per-point outputs every tile is evaluated, without them the tiles behind
    the first hit are not.  Rays that hit in the first, a middle and no tile, negative and non-finite lengths behind the hit."""
    f = _field(net, cuda0)
    o, d, ln = rr.bundle(9, 200, zero_dir=False)
    ln[3, 150:] *= -1.0
    ln[4, 190] = np.nan
    ln[5, 199] = np.inf
    o[6] = 40.0                                      # far outside: whatever it hits, it is evaluated to the end
    full = _dev(f, o, d, ln, 0.2)
    lean = _dev(f, o, d, ln, 0.2, densities=False, colours=False)
    _same(lean, full, ("image", "depth", "points", "hit", "weights"))
    first = np.argmax(full["weights"] != 0, axis=1)
    assert (first[full["hit"] != 0] < 128).any()      # some ray does leave tiles unevaluated
    _same(full, rr.host_field(net)[0].render_host(o, d, ln, 0.2))


@pytest.mark.parametrize("threshold", [0.2, -1.0])
def test_fused_image_equals_ea_march_of_its_own_outputs(cuda0, threshold):
    f = _field(rr.NETS[3], cuda0)                    # C = 32
    o, d, ln = rr.bundle(70, 33)
    t = lambda a: torch.from_numpy(a).to(cuda0)
    out = ops.radiance_render(f.rpack, f.widths, f.H, f.Wc, f.C, t(o), t(d), t(ln), threshold=threshold, want_weights=True,
                              want_densities=True, want_colours=True)
    image, wts = ops.ea_march(out["densities"], out["colours"], threshold)
    assert rr.same(image.cpu().numpy(), out["image"].cpu().numpy()) and rr.same(wts.cpu().numpy(), out["weights"].cpu().numpy())


@pytest.mark.parametrize("F", [1, 12, 13, 64])
def test_ea_march_equals_the_host_build(cuda0, F):
    rng = np.random.default_rng(F)
    for N, P, thr in ((1, 1, -1.0), (300, 33, -1.0), (257, 65, 0.2)):
        rho = rng.uniform(0, 0.6, (N, P)).astype(f32)
        rho[0] = 0.0
        rho[N // 2, P // 2] = np.nan
        feats = rng.standard_normal((N, P, F)).astype(f32)
        image, wts = ops.ea_march(torch.from_numpy(rho).to(cuda0), torch.from_numpy(feats).to(cuda0), thr)
        want_image, want_wts = ops.ea_march_host(rho, feats, thr)
        assert rr.same(image.cpu().numpy(), want_image) and rr.same(wts.cpu().numpy(), want_wts)
        image2, none = ops.ea_march(torch.from_numpy(rho).to(cuda0), torch.from_numpy(feats).to(cuda0), thr, want_weights=False)
        assert none is None and rr.same(image2.cpu().numpy(), want_image)
    m = rays.EmissionAbsorptionRaymarcherStratified(thresholdMode=True, threshold=0.2)
    image3, wts3 = m(torch.from_numpy(rho).to(cuda0).reshape(1, N, P, 1), torch.from_numpy(feats).to(cuda0).reshape(1, N, P, F))
    assert image3.shape == (1, N, F + 1) and wts3.shape == (1, N, P) and rr.same(image3.cpu().numpy()[0], want_image)


@pytest.mark.parametrize("threshold", [0.2, -1.0])
@pytest.mark.parametrize("P,N", [(2, 70), (100, 5)])
def test_density_outputs_equal_density_march(cuda0, P, N, threshold):
    f = _field(rr.NETS[2], cuda0)
    o, d, ln = rr.bundle(N, P)
    t = lambda a: torch.from_numpy(a).to(cuda0)
    got = _dev(f, o, d, ln, threshold)
    pts, depth, hit, rho, w = ops.density_march(f.pack, f.widths, f.H, t(o), t(d), t(ln), threshold, want_densities=True,
                                                want_weights=True)
    for k, v in (("points", pts), ("depth", depth), ("hit", hit), ("densities", rho), ("weights", w)):
        assert rr.same(got[k], v.cpu().numpy()), k
    b = SimpleNamespace(origins=t(o), directions=t(d), lengths=t(ln))
    dens, zeros = f.batched_forward_fordensity(b)      # what DensityField offers keeps working
    assert rr.same(dens.cpu().numpy()[..., 0], got["densities"]) and zeros.shape == (N, P, 3)
    images, wts, dep = f.render(b, threshold=threshold)
    assert images.shape == (N, f.C + 1) and wts.shape == (N, P) and dep.shape == (N,)
    assert rr.same(images.cpu().numpy(), got["image"]) and rr.same(dep.cpu().numpy(), got["depth"])
    assert f.render(b, threshold=threshold, return_weights=False)[1] is None


def test_rows_are_independent(cuda0):
    f = _field(rr.NETS[1], cuda0)
    for P in (3, 70):
        o, d, ln = rr.bundle(4097, P, zero_dir=False)
        big = _dev(f, o, d, ln, -1.0)
        for i in (0, 2048, 4096):
            one = _dev(f, o[i:i + 1], d[i:i + 1], ln[i:i + 1], -1.0)
            for k in KEYS:
                assert rr.same(one[k], big[k][i:i + 1]), (k, i)


@pytest.mark.parametrize("threshold", [0.2, -1.0])
def test_non_finite_rays_poison_only_themselves(cuda0, threshold):
    f = _field(rr.NETS[1], cuda0)
    for P in (2, 70):
        o, d, ln = rr.bundle(40, P, zero_dir=False)
        clean = _dev(f, o, d, ln, threshold)
        o2, d2 = o.copy(), d.copy()
        o2[3, 1] = np.nan
        d2[7, 0] = np.inf
        d2[11] = np.nan
        o2[39, 2] = -np.inf
        got = _dev(f, o2, d2, ln, threshold)
        keep = np.setdiff1d(np.arange(40), [3, 7, 11, 39])
        for k in KEYS:
            assert rr.same(got[k][keep], clean[k][keep]), k
        for i in (3, 7, 11, 39):
            assert np.isnan(got["image"][i, :f.C]).all() and np.isnan(got["colours"][i]).all() and got["hit"][i] in (0, 1)
        _same(got, rr.host_field(rr.NETS[1])[0].render_host(o2, d2, ln, threshold))


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_every_output_is_written_whatever_the_buffers_held(cuda0, monkeypatch, byte):
    f = _field(rr.NETS[0], cuda0)
    for P, N in ((2, 70), (70, 3)):
        o, d, ln = rr.bundle(N, P)
        want = rr.host_field(rr.NETS[0])[0].render_host(o, d, ln, 0.2)
        with poison.poisoned(monkeypatch, byte):
            got = _dev(f, o, d, ln, 0.2)
            lean = _dev(f, o, d, ln, 0.2, weights=False, densities=False, colours=False)
            rho, feats = torch.from_numpy(want["densities"]).to(cuda0), torch.from_numpy(want["colours"]).to(cuda0)
            image, wts = (x.cpu().numpy() for x in ops.ea_march(rho, feats, 0.2))
        _same(got, want)
        _same(lean, want)
        assert lean["weights"] is None and lean["densities"] is None and lean["colours"] is None
        assert rr.same(image, want["image"]) and rr.same(wts, want["weights"])


def test_null_outputs_workspace_reuse_and_streams(cuda0):
    f = _field(rr.NETS[1], cuda0)
    o, d, ln = rr.bundle(130, 5)
    want = rr.host_field(rr.NETS[1])[0].render_host(o, d, ln, -1.0)
    need = ops.radiance_workspace_bytes(130, f.Wc)
    assert need == 130 * 64 * 4
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=cuda0)
    _same(_dev(f, o, d, ln, -1.0, workspace=ws), want)
    assert bool((ws[need:] == 0xFF).all())            # nothing behind the stated size is touched
    _same(_dev(f, o[:9], d[:9], ln[:9], -1.0, workspace=ws), {k: v[:9] for k, v in want.items()})      # reused, second call
    stream = torch.cuda.Stream(device=cuda0)
    with torch.cuda.stream(stream):
        got = _dev(f, o, d, ln, -1.0, colours=False)
    stream.synchronize()
    _same(got, want)
    empty = ops.radiance_render(f.rpack, f.widths, f.H, f.Wc, f.C, torch.empty((0, 3), device=cuda0), torch.empty((0, 3), device=cuda0),
                                torch.empty((0, 5), device=cuda0), want_weights=True)
    assert empty["image"].shape == (0, f.C + 1) and empty["weights"].shape == (0, 5)


def test_refusals_launch_nothing(cuda0, hip_lib):
    f = _field(rr.NETS[1], cuda0)
    o, d, ln = (torch.from_numpy(a).to(cuda0) for a in rr.bundle(4, 3))
    ws = torch.empty((16,), dtype=torch.uint8, device=cuda0)      # short
    sentinel = torch.full((4, f.C + 1), 7.0, device=cuda0)
    w = (ctypes.c_int32 * 2)(*f.widths)
    args = lambda P=3, thr=0.2, wsb=16, C=f.C: (f.rpack.data_ptr(), f.rpack.numel() * 4, 2, ctypes.cast(w, ctypes.c_void_p), f.H, f.Wc, C,
                                               o.data_ptr(), d.data_ptr(), ln.data_ptr(), 4, P, thr, sentinel.data_ptr(),
                                               sentinel.data_ptr(), sentinel.data_ptr(), sentinel.data_ptr(), None, None, None,
                                               ws.data_ptr(), wsb, None)
    for bad in (args(), args(P=0), args(thr=float("nan")), args(C=33), args(wsb=0)):
        assert hip_lib.isr_radiance_render(*bad) < 0 and hip_lib.isr_last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())
    with pytest.raises(_capi.IsrError):
        ops.radiance_render(f.rpack, f.widths, f.H, f.Wc, f.C, o, d, ln, workspace=ws)
    with pytest.raises(ValueError):
        ops.radiance_render(f.rpack, f.widths, f.H, f.Wc, f.C, o, d[:3], ln)
    with pytest.raises(ValueError):
        ops.ea_march(torch.zeros((2, 3), device=cuda0), torch.zeros((2, 4, 5), device=cuda0))


def _grid_setup(cuda0):
    R = torch.eye(3)[None]
    T = torch.tensor([[0.0, 0.0, 2.5]])
    cams = rays.PerspectiveCameras(R, T, focal_length=2.0, in_ndc=True, device=cuda0)
    sampler = rays.NDCMultinomialRaysampler(8, 8, 70, 1.0, 4.0)
    mask = torch.zeros((1, 8, 8, 1), device=cuda0)
    mask[0, 1:7, 2:6] = 1
    return cams, sampler, mask


@pytest.mark.parametrize("threshold_mode", [False, True])
def test_renderer_fused_equals_generic(cuda0, threshold_mode):
    f = _field(rr.NETS[1], cuda0)
    cams, sampler, mask = _grid_setup(cuda0)
    marcher = rays.EmissionAbsorptionRaymarcherStratified(thresholdMode=threshold_mode, threshold=0.2)
    r = rays.ImplicitRendererStratified(sampler, marcher, device=cuda0)
    for kw, lead in ((dict(), (1, 8, 8)), (dict(maskRays=True, mask=mask), (1, 24))):
        fused = r(cams, f.batched_forward, **kw)
        generic = r(cams, lambda ray_bundle, **k: f.batched_forward(ray_bundle, **k), **kw)
        assert fused[0].shape == (*lead, f.C + 1) and fused[2].shape == (*lead, 70) and fused[1].lengths.shape == (*lead, 70)
        assert rr.same(fused[0].cpu().numpy(), generic[0].cpu().numpy()) and rr.same(fused[2].cpu().numpy(), generic[2].cpu().numpy())
        b = fused[1]
        want = rr.host_field(rr.NETS[1])[0].render_host(b.origins.cpu().numpy().reshape(-1, 3), b.directions.cpu().numpy().reshape(-1, 3),
                                                        b.lengths.cpu().numpy().reshape(-1, 70), 0.2 if threshold_mode else -1.0)
        assert rr.same(fused[0].cpu().numpy().reshape(-1, f.C + 1), want["image"])
    image, silhouette = render.full_render(f, cams, r)
    assert image.shape == (8, 8, f.C) and silhouette.shape == (8, 8, 1)


def test_feature_field_route_equals_its_composition(cuda0):
    net = rr.NETS[1]
    Ws, bs, _, _ = rr.fixture(*net)
    dens = DensityField(Ws, bs, dr.frequencies(net[0]), 10.0, cuda0)
    rng = np.random.default_rng(5)
    kw = [rng.uniform(-1, 1, (o, i)).astype(f32) / np.sqrt(i).astype(f32) for i, o in ((3, 64), (64, 64), (64, 12))]
    kb = [rng.uniform(-0.1, 0.1, o).astype(f32) for o in (64, 64, 12)]
    keys = KeyField(kw, kb, [30.0, 30.0, None], cuda0)
    cams, sampler, mask = _grid_setup(cuda0)
    marcher = rays.EmissionAbsorptionRaymarcherStratified(thresholdMode=True, threshold=0.2)
    r = rays.ImplicitRendererStratified(sampler, marcher, device=cuda0)
    images, b, weights = r(cams, FeatureField(dens, keys).batched_forward, maskRays=True, mask=mask)
    assert images.shape == (1, 24, 13) and weights.shape == (1, 24, 70)
    o, d, ln = (x.cpu().numpy().reshape(24, -1) for x in (b.origins, b.directions, b.lengths))
    rho = dens.march_host(o, d, ln, 0.2)["densities"]
    pts = (b.origins[..., None, :] + b.lengths[..., :, None] * b.directions[..., None, :]).cpu().numpy().reshape(-1, 3)
    want_image, want_wts = ops.ea_march_host(rho, keys.eval_host(pts).reshape(24, 70, 12), 0.2)
    assert rr.same(images.cpu().numpy()[0], want_image) and rr.same(weights.cpu().numpy()[0], want_wts)


def test_from_module_and_from_linears(cuda0):
    net = rr.NETS[0]
    weights = rr.fixture(*net)
    tm = rr.TorchRadiance(weights, dr.frequencies(net[0])).to(cuda0)
    tm.harmonic_embedding = SimpleNamespace(frequencies=tm.frequencies)
    a = RadianceField.from_module(tm)
    b = RadianceField.from_linears([tm.mlp[0]], tm.density_layer[0], [tm.color_layer[0], tm.color_layer[2]], n_harmonic=net[0])
    ref = rr.host_field(net)[0]
    for f in (a, b):
        assert f.device == cuda0 and np.array_equal(rr.bits(f.rpack_host), rr.bits(ref.rpack_host))


@pytest.mark.parametrize("tag", ["big", "small"])
def test_reference_fixture_on_the_device(cuda0, tag):
    """tests/test_ref_radiance_cpu.py's conditions on the device's results, which are the host build's bits."""
    from tests import ref_fields as rf
    g = rf.load("ref_radiance_render")
    f = rr.ref_field(tag, cuda0)
    o, d, ln = g[f"{tag}_origins"][0], g[f"{tag}_directions"][0], g[f"{tag}_lengths"][0]
    soft, thr = _dev(f, o, d, ln, -1.0), _dev(f, o, d, ln, rr.THRESHOLD)
    rr.check_against_reference(tag, soft, thr, "device")
    host = rr.ref_field(tag)
    _same(soft, host.render_host(o, d, ln, -1.0))
    _same(thr, host.render_host(o, d, ln, rr.THRESHOLD))
