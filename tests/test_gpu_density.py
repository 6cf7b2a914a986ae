"""GPU: isr_density_eval / isr_density_march against the host build of the same header (bit for bit), row independence,
non-finite inputs, outputs written whatever the buffers held, and the route from a DensityField to export_keys."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import key_export, ops, render, synth
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField, KeyField
from tests import density_ref as dr
from tests import field_ref, poison

pytestmark = pytest.mark.gpu
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)

_cache = {}


def _field(H, hidden, n_layers, dev, seed=None):
    key = (H, hidden, n_layers, seed)
    if key not in _cache:
        Ws, bs = dr.fixture(H, hidden, n_layers, H + hidden + n_layers if seed is None else seed)
        _cache[key] = DensityField(Ws, bs, dr.frequencies(H), 10.0, dev)
    return _cache[key]


def _rays(R, P, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.5, 0.5, (R, 3)).astype(np.float32)
    d = rng.normal(size=(R, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = np.sort(rng.uniform(0.0, 1.5, (R, P)).astype(np.float32), axis=1)
    return o, d, ln


def _march_dev(f, o, d, ln, thr, dens, wts=True):
    t = lambda a: torch.from_numpy(a).to(f.device)
    pts, depth, hit, rho, w = ops.density_march(f.pack, f.widths, f.H, t(o), t(d), t(ln), thr, want_densities=dens, want_weights=wts)
    c = lambda x: None if x is None else x.cpu().numpy()
    return dict(points=c(pts), depth=c(depth), hit=c(hit), densities=c(rho), weights=c(w))


def _same(got, want, dens=True):
    for k in ("points", "depth", "weights") + (("densities",) if dens else ()):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(got["hit"], want["hit"])


@pytest.mark.parametrize("H,hidden,n_layers,N", [(1, 32, 1, 1), (1, 32, 2, 63), (4, 32, 1, 65), (4, 256, 2, 63), (60, 32, 2, 65),
                                                 (60, 256, 1, 257), (60, 256, 2, 257), (1, 256, 1, 257), (4, 32, 2, 257),
                                                 (4, 128, 2, 65), (4, 160, 1, 63), (4, 100, 2, 65), (1, 33, 1, 63)])
def test_eval_equals_the_host_build(cuda0, H, hidden, n_layers, N):
    """The last row: 4 blocks of 32 neurons (the most that go one 32 x 32 tile per wave) and 5 (one block per wave, three waves
    idle); widths that are no multiple of 32 or 8, whose padded neurons feed the next layer as zeros."""
    f = _field(H, hidden, n_layers, cuda0)
    pts = np.random.default_rng(N).uniform(-1.2, 1.2, (N, 3)).astype(np.float32)
    got = f.customForwardForDensity(torch.from_numpy(pts).to(cuda0))
    assert got.shape == (N, 1)
    want = f.eval_host(pts)
    assert np.array_equal(bits(got.cpu().numpy().reshape(-1)), bits(want))
    if N >= 63:
        assert 0.2 <= float((want > 0.2).mean()) <= 0.8


@pytest.mark.parametrize("threshold", [0.2, -1.0])
@pytest.mark.parametrize("P,R", [(1, 130), (2, 5), (33, 5), (33, 130), (128, 1), (128, 5), (100, 3)])
def test_march_equals_the_host_build(cuda0, P, R, threshold):
    """P = 1, 2, 33: several rays per workgroup (ragged last group); 33 and 100: a ray's points are no multiple of the tile;
    100, 128: a ray split across tiles.  With and without the densities (without, threshold mode stops after the first hit)."""
    f = _field(4, 32, 1, cuda0, seed=3)
    o, d, ln = _rays(R, P, 100 * P + R)
    if R >= 5:
        ln[1] = -ln[1]
        ln[2, 0] = 0.0
    want = f.march_host(o, d, ln, threshold)
    _same(_march_dev(f, o, d, ln, threshold, True), want)
    _same(_march_dev(f, o, d, ln, threshold, False), want, dens=False)


def test_reference_width_march(cuda0):
    """H = 60, 256-256-1, 4 096 rays x 32 points, both modes, against the host build."""
    f = _field(60, 256, 2, cuda0)
    o, d, ln = _rays(4096, 32, 77)
    want = f.march_host(o, d, ln, 0.2)
    assert 0.2 <= float((want["densities"] > 0.2).mean()) <= 0.8
    _same(_march_dev(f, o, d, ln, 0.2, True), want)
    _same(_march_dev(f, o, d, ln, 0.2, False), want, dens=False)
    soft = _march_dev(f, o, d, ln, -1.0, True)
    assert np.array_equal(bits(soft["densities"]), bits(want["densities"]))
    wts, depth, hit = dr.march(ln[:64], want["densities"][:64], -1.0)
    assert np.array_equal(bits(soft["weights"][:64]), bits(wts)) and np.array_equal(bits(soft["depth"][:64]), bits(depth))


def test_rows_are_independent(cuda0):
    f = _field(60, 256, 2, cuda0)
    pts = torch.from_numpy(np.random.default_rng(1).uniform(-1.2, 1.2, (300, 3)).astype(np.float32)).to(cuda0)
    whole = f.customForwardForDensity(pts)
    for sl in (slice(0, 1), slice(5, 70), slice(299, 300), slice(64, 128)):
        assert torch.equal(whole[sl].view(torch.int32), f.customForwardForDensity(pts[sl].contiguous()).view(torch.int32))
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(0)).to(cuda0)
    assert torch.equal(whole[perm].view(torch.int32), f.customForwardForDensity(pts[perm]).view(torch.int32))
    o, d, ln = _rays(10, 24, 5)
    rb = SimpleNamespace(origins=torch.from_numpy(o).to(cuda0)[None], directions=torch.from_numpy(d).to(cuda0)[None],
                         lengths=torch.from_numpy(ln).to(cuda0)[None])
    d16, z16 = f.batched_forward_fordensity(rb)
    d3, _ = f.batched_forward_fordensity(rb, n_batches=3)
    assert d16.shape == (1, 10, 24, 1) and z16.shape == (1, 10, 24, 3) and not z16.any()
    assert torch.equal(d16.view(torch.int32), d3.view(torch.int32))
    world = rb.origins[..., None, :] + rb.directions[..., None, :] * rb.lengths[..., :, None]
    assert torch.equal(d16.view(torch.int32), f.customForwardForDensity(world).view(torch.int32))


def test_non_finite_coordinates_poison_only_their_own(cuda0):
    f = _field(4, 32, 2, cuda0)
    pts = np.random.default_rng(2).uniform(-1, 1, (130, 3)).astype(np.float32)
    clean = f.customForwardForDensity(torch.from_numpy(pts).to(cuda0)).cpu().numpy().reshape(-1)
    bad = pts.copy()
    bad[3, 0], bad[64, 1], bad[129, 2] = np.nan, np.inf, -np.inf
    got = f.customForwardForDensity(torch.from_numpy(bad).to(cuda0)).cpu().numpy().reshape(-1)
    rows = np.array([3, 64, 129])
    assert np.isnan(got[rows]).all()
    keep = np.setdiff1d(np.arange(130), rows)
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    o, d, ln = _rays(9, 20, 3)
    clean = _march_dev(f, o, d, ln, -1.0, True)
    o2 = o.copy()
    o2[4, 1] = np.nan
    got = _march_dev(f, o2, d, ln, -1.0, True)
    keep = np.setdiff1d(np.arange(9), [4])
    for k in ("points", "depth", "weights", "densities"):
        assert np.array_equal(bits(got[k][keep]), bits(clean[k][keep])), k
        assert np.isnan(got[k][4]).all(), k
    want = f.march_host(o2, d, ln, -1.0)             # a NaN is a NaN on both builds; its sign and payload are the hardware's
    for k in ("points", "depth", "weights", "densities"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
        assert np.array_equal(bits(got[k])[~np.isnan(want[k])], bits(want[k])[~np.isnan(want[k])]), k
    assert np.array_equal(got["hit"], want["hit"]) and got["hit"][4] == 1


def test_every_output_is_written_whatever_the_buffers_held(cuda0, monkeypatch):
    f = _field(4, 32, 1, cuda0, seed=3)
    o, d, ln = _rays(70, 100, 8)
    t = lambda a: torch.from_numpy(a).to(cuda0)
    to, td, tl, tp = t(o), t(d), t(ln), t(o)

    def run():
        return (ops.density_eval(f.pack, f.widths, f.H, tp),
                ops.density_march(f.pack, f.widths, f.H, to, td, tl, 0.2, want_densities=True, want_weights=True),
                ops.density_march(f.pack, f.widths, f.H, to, td, tl, 0.2),
                ops.density_march(f.pack, f.widths, f.H, to, td, tl, -1.0),
                ops.density_march(f.pack, f.widths, f.H, to, td, tl, 2.0, want_weights=True))       # no ray hits anything

    a, b = poison.run_twice(monkeypatch, run)
    assert poison.same_bits(a, b)
    want = f.march_host(o, d, ln, 0.2)
    pts, depth, hit, rho, w = a[1]
    _same(dict(points=pts.numpy(), depth=depth.numpy(), hit=hit.numpy(), densities=rho.numpy(), weights=w.numpy()), want)
    assert a[2][3] is None and a[2][4] is None
    assert np.array_equal(bits(a[2][0].numpy()), bits(want["points"])) and np.array_equal(a[2][2].numpy(), want["hit"])
    none = a[4]
    assert not none[2].any() and not none[4].any() and torch.equal(none[0], torch.from_numpy(o)) and not none[1].any()


def test_null_densities_and_weights_touch_nothing_else(cuda0):
    """One allocation, the three outputs in its middle: the words around them keep their pattern."""
    f = _field(4, 32, 1, cuda0, seed=3)
    o, d, ln = _rays(33, 70, 4)
    t = lambda a: torch.from_numpy(a).to(cuda0)
    to, td, tl = t(o), t(d), t(ln)
    from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import check, current_stream, lib, ptr
    import ctypes
    N, P, pad = 33, 70, 4096
    buf = torch.full((pad + 5 * N + pad,), 12345.0, dtype=torch.float32, device=cuda0)
    depth, points, hit = buf[pad:pad + N], buf[pad + N:pad + 4 * N], buf[pad + 4 * N:pad + 5 * N]
    w = (ctypes.c_int32 * 1)(32)
    check(lib().isr_density_march(ptr(f.pack), f.pack.numel() * 4, 1, ctypes.cast(w, ctypes.c_void_p), 4, ptr(to), ptr(td), ptr(tl),
                                  N, P, 0.2, None, None, ptr(depth), ptr(points), ptr(hit), current_stream(cuda0)),
          "isr_density_march")
    torch.cuda.synchronize()
    assert bool((buf[:pad] == 12345.0).all()) and bool((buf[pad + 5 * N:] == 12345.0).all())
    want = f.march_host(o, d, ln, 0.2)
    assert np.array_equal(bits(depth.cpu().numpy()), bits(want["depth"]))
    assert np.array_equal(bits(points.cpu().numpy().reshape(N, 3)), bits(want["points"]))
    assert np.array_equal(hit.view(torch.int32).cpu().numpy(), want["hit"])


def test_refusals_on_the_device(cuda0):
    f = _field(4, 32, 1, cuda0, seed=3)
    z3, z = torch.zeros(4, 3, device=cuda0), torch.zeros(4, 2, device=cuda0)
    with pytest.raises(ValueError):
        ops.density_march(f.pack, f.widths, f.H, z3, z3, torch.zeros(4, 0, device=cuda0))
    with pytest.raises(ValueError):
        ops.density_march(f.pack, f.widths, f.H, z3, z3, torch.zeros(2, 4, device=cuda0).t())
    with pytest.raises(ValueError):
        ops.density_march(f.pack, f.widths, f.H, z3.double(), z3, z)
    with pytest.raises(ValueError):
        ops.density_eval(f.pack, f.widths, f.H, torch.zeros(3, 4, device=cuda0).t())
    with pytest.raises(ValueError):
        f.surface_points(z3, z3, z, surface_thickness=2)
    assert ops.density_eval(f.pack, f.widths, f.H, torch.zeros(0, 3, device=cuda0)).shape == (0,)


def test_grid_densities_order(cuda0):
    f = _field(4, 32, 1, cuda0, seed=3)
    res = 8
    g = f.grid_densities(res)
    assert g.shape == (res, res, res)
    flat = f.customForwardForDensity(torch.from_numpy(dr.grid_points(res)).to(cuda0)).view(res, res, res)
    assert torch.equal(g.view(torch.int32), flat.movedim(0, 2).movedim(1, 0).contiguous().view(torch.int32))


def test_surface_points_to_export_keys_end_to_end(cuda0):
    """Rays through a small density field, the candidates into export_keys with synth's torus as the mesh and a small KeyField
    (the field is random, so max_dist is wide: what is checked is that every stage takes the one before it)."""
    f = _field(4, 32, 1, cuda0, seed=3)
    bundles = []
    for s in range(2):
        o, d, ln = _rays(600, 24, 40 + s)
        bundles.append(SimpleNamespace(origins=torch.from_numpy(o).to(cuda0)[None], directions=torch.from_numpy(d).to(cuda0)[None],
                                       lengths=torch.from_numpy(ln).to(cuda0)[None]))
    pts, depth, hit, wts = f.surface_points(bundles[0].origins, bundles[0].directions, bundles[0].lengths, return_weights=True)
    assert pts.shape == (1, 600, 3) and depth.shape == (1, 600) and hit.dtype == torch.bool and wts.shape == (1, 600, 24)
    assert torch.equal(hit, (wts != 0).any(dim=-1)) and 0 < int(hit.sum()) < 600
    cand = key_export.collect_candidates(f, bundles)
    moved = sum(int(((f.surface_points(b.origins, b.directions, b.lengths)[0] - b.origins).norm(dim=-1) != 0).sum()) for b in bundles)
    assert cand.shape == (moved, 3) and cand.is_cuda and moved > 100
    v, tri = synth.make_mesh("torus", 32, radius=0.5 / 1.4, tube=0.4)
    mesh = render.Mesh(v, tri)
    Ws, bs = field_ref.siren_params((3, 16, 6), (30.0, None), seed=1)
    kf = KeyField(Ws, bs, (30.0, None), cuda0)
    scaled, feats, normals, kept = key_export.export_keys(cand, mesh, kf, diameter=100.0, K=64, box=3.0, max_dist=5.0)
    assert len(kept) > 0 and scaled.shape == (len(kept), 3) and feats.shape == (len(kept), 6) and normals.shape == (len(kept), 3)
    assert np.array_equal(scaled, cand.cpu().numpy()[kept] * np.float32(100.0 / 1.8))
