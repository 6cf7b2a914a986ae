"""The radiance field's backward on the device (include/isr_radiance_grad.h): isr_radiance_backward against the host build of
the same header bit for bit, the device-side packing, buffer hygiene, the autograd route of fields.TrainableRadianceField,
torch autograd on the device as the yardstick, and training.nerf_train_step with two trainable fields."""
import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, fields, ops, rays, training
from tests import density_ref as dr
from tests import poison
from tests import radiance_grad_ref as gr
from tests import radiance_ref as rr

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SMALL = [n for n in gr.FIELDS if n != gr.REFERENCE]


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _packs(name, dev):
    """-> (pack, packT) by isr_radiance_pack_device from the field's weights on the device."""
    _, w = gr.host_field(name)
    W = _dev(np.concatenate([a.reshape(-1) for a in (*w[0], *w[2])]), dev)
    b = _dev(np.concatenate([*w[1], *w[3]]), dev)
    return ops.radiance_pack_device(*gr.shape_args(name), dr.frequencies(gr.FIELDS[name][0]), gr.BETA, W, b)


def _device_backward(name, dev, o, d, ln, dd, dc, packs=None, **kw):
    pack, packT = packs or _packs(name, dev)
    dW, db = ops.radiance_backward(pack, packT, *gr.shape_args(name), _dev(o, dev), _dev(d, dev), _dev(ln, dev), _dev(dd, dev),
                                   _dev(dc, dev), **kw)
    return (None if dW is None else dW.cpu().numpy()), (None if db is None else db.cpu().numpy())


def _case(name, N, P, kind="random", seed=0):
    o, d, ln = rr.bundle(N, P, seed)
    return (o, d, ln, *gr.upstream(N, P, gr.FIELDS[name][3], kind, seed))


@pytest.mark.parametrize("name", list(gr.FIELDS))
def test_device_is_host_bit_for_bit(cuda0, name):
    """Every field at every shape edge (the reference's at a handful of points), and every upstream case at one shape."""
    packs = _packs(name, cuda0)
    shapes = gr.SHAPES if name != gr.REFERENCE else ((0, 3), (5, 13), (2, 65))
    cases = [(N, P, "random") for N, P in shapes] + [(5, 13, k) for k in gr.UPSTREAMS if name != gr.REFERENCE]
    for N, P, kind in cases:
        c = _case(name, N, P, kind)
        hW, hb = gr.host_backward(name, *c)
        gW, gb = _device_backward(name, cuda0, *c, packs=packs)
        assert gr.same(gW, hW) and gr.same(gb, hb), (name, N, P, kind)
        if kind in ("zeros", "both null") or N == 0:
            assert not gW.view(np.uint32).any() and not gb.view(np.uint32).any(), (name, N, P, kind)      # exactly +0


@pytest.mark.parametrize("name", ["H4 5 Wc5 C3", "H4 32-33 Wc40 C3"])
def test_sizes_past_a_batch_and_a_slab(cuda0, name):
    geo = ops.radiance_grad_geometry()
    assert geo["chain"] == 64 and geo["batch"] % geo["chain"] == 0 and geo["slab"] % geo["batch"] == 0
    packs = _packs(name, cuda0)
    for points, P in ((4097, 17), (geo["batch"] + 1, 3), (geo["slab"] + 1, 5)):
        assert points % P == 0
        c = _case(name, points // P, P)
        hW, hb = gr.host_backward(name, *c)
        gW, gb = _device_backward(name, cuda0, *c, packs=packs)
        assert gr.same(gW, hW) and gr.same(gb, hb), (name, points, P)


def test_reference_widths_and_forced_slabs(cuda0):
    """The reference's widths at 4 097 points: the host's bits; and through slabs of 64 and 1 024 points the same bits again."""
    name = gr.REFERENCE
    packs = _packs(name, cuda0)
    c = _case(name, 241, 17)
    hW, hb = gr.host_backward(name, *c)
    gW, gb = _device_backward(name, cuda0, *c, packs=packs)
    assert gr.same(gW, hW) and gr.same(gb, hb)
    for slab in (64, 1024):
        sW, sb = _device_backward(name, cuda0, *c, packs=packs, slab=slab)
        assert gr.same(sW, gW) and gr.same(sb, gb), slab


@pytest.mark.parametrize("name", list(gr.FIELDS))
def test_device_pack(cuda0, name, monkeypatch):
    """pack is isr_radiance_pack's bytes; packT is the restated transposed pack; every word of both is written whatever
    the buffers held."""
    fld, w = gr.host_field(name)
    a, b = poison.run_twice(monkeypatch, lambda: _packs(name, cuda0))
    assert poison.same_bits(a, b)
    assert np.array_equal(a[0].numpy().view(np.uint32), fld.rpack_host.view(np.uint32))
    assert np.array_equal(a[1].numpy().view(np.uint32), gr.pack_t(w).view(np.uint32))
    zero = torch.zeros_like(a[0], device=cuda0), torch.zeros_like(a[1], device=cuda0)
    W = _dev(np.concatenate([x.reshape(-1) for x in (*w[0], *w[2])]), cuda0)
    bb = _dev(np.concatenate([*w[1], *w[3]]), cuda0)
    ops.radiance_pack_device(*gr.shape_args(name), dr.frequencies(gr.FIELDS[name][0]), gr.BETA, W, bb, *zero)
    assert poison.same_bits((zero[0].cpu(), zero[1].cpu()), a)


def test_buffer_hygiene_and_call_variants(cuda0, monkeypatch):
    name = "H4 32-33 Wc40 C3"
    c = _case(name, 43, 3)
    hW, hb = gr.host_backward(name, *c)
    run = lambda **kw: _device_backward(name, cuda0, *c, **kw)
    a, b = poison.run_twice(monkeypatch, run)                  # outputs, packs and the workspace under 0xFF, then 0x7F
    with poison.poisoned(monkeypatch, 0x00):                   # and under 0x00
        c0 = run()
    for gW, gb in (a, b, c0):
        assert gr.same(gW, hW) and gr.same(gb, hb)
    packs = _packs(name, cuda0)
    shape = gr.shape_args(name)
    widths = np.asarray(shape[0], np.int32)
    ws_bytes = _capi.lib().isr_radiance_grad_workspace_bytes(len(widths), widths.ctypes.data, *shape[1:], 43, 3)
    assert ws_bytes > 0
    for byte in (0x00, 0x7F, 0xFF):                            # a caller's workspace, pre-filled and reused
        ws = torch.full((ws_bytes,), byte, dtype=torch.uint8, device=cuda0)
        for _ in range(2):
            gW, gb = run(packs=packs, workspace_buf=ws)
            assert gr.same(gW, hW) and gr.same(gb, hb), byte
    stream = torch.cuda.Stream(cuda0)                          # a caller's stream
    with torch.cuda.stream(stream):
        gW, gb = run(packs=packs)
    stream.synchronize()
    assert gr.same(gW, hW) and gr.same(gb, hb)
    gW, gb = run(packs=packs, need=(True, False))              # each of dW, db left out
    assert gb is None and gr.same(gW, hW)
    gW, gb = run(packs=packs, need=(False, True))
    assert gW is None and gr.same(gb, hb)
    for kind in ("densities only", "colours only"):            # each upstream left out: the same as zeros in its place
        k = _case(name, 43, 3, kind)
        z = [np.zeros((43, 3), f32) if k[3] is None else k[3], np.zeros((43, 3, 3), f32) if k[4] is None else k[4]]
        assert all(gr.same(x, y) for x, y in zip(_device_backward(name, cuda0, *k, packs=packs),
                                                 _device_backward(name, cuda0, *k[:3], *z, packs=packs)))
    with poison.poisoned(monkeypatch, 0xFF):                   # N = 0 writes zeros
        gW, gb = _device_backward(name, cuda0, *_case(name, 0, 3), packs=packs)
    assert not gW.any() and not gb.any() and not np.isnan(gW).any()


def test_refusals(cuda0):
    name = "H4 5 Wc5 C3"
    pack, packT = _packs(name, cuda0)
    shape = gr.shape_args(name)
    o, d, ln, dd, dc = (_dev(a, cuda0) for a in _case(name, 5, 13))
    with pytest.raises(_capi.IsrError):                        # a short workspace
        ops.radiance_backward(pack, packT, *shape, o, d, ln, dd, dc, workspace_buf=torch.empty(256, dtype=torch.uint8, device=cuda0))
    with pytest.raises(_capi.IsrError):                        # another field's transposed pack
        ops.radiance_backward(pack, packT[:-32].contiguous(), *shape, o, d, ln, dd, dc)
    with pytest.raises(_capi.IsrError):                        # P beyond isr_radiance_render's
        big = torch.zeros((1, 4097), device=cuda0)
        ops.radiance_backward(pack, packT, *shape, o[:1].contiguous(), d[:1].contiguous(), big, None, None)
    with pytest.raises(_capi.IsrError):                        # a shape isr_radiance_render refuses
        ops.radiance_backward(pack, packT, shape[0], shape[1], 300, shape[3], o, d, ln, None, None)
    with pytest.raises(ValueError):
        ops.radiance_backward(pack, packT, *shape, o, d, ln, dd[:, :5].contiguous(), dc)
    with pytest.raises(ValueError):
        ops.radiance_backward(pack, packT, *shape, o, d, ln, dd, dc, slab=100)
    L = _capi.lib()
    w = np.asarray(shape[0], np.int32)
    assert L.isr_radiance_backward(pack.data_ptr(), pack.numel() * 4, packT.data_ptr(), packT.numel() * 4, 1, w.ctypes.data, *shape[1:],
                                   o.data_ptr(), d.data_ptr(), ln.data_ptr(), 5, 13, None, None, None, None, None, 0, None) != 0      # null workspace
    assert L.isr_radiance_backward(pack.data_ptr(), pack.numel() * 4, packT.data_ptr(), packT.numel() * 4, 1, w.ctypes.data, *shape[1:],
                                   None, d.data_ptr(), ln.data_ptr(), 5, 13, None, None, None, None, None, 0, None) != 0               # null rays


def _trainable(name, dev):
    _, w = gr.host_field(name)
    return fields.TrainableRadianceField(*w, dr.frequencies(gr.FIELDS[name][0]), gr.BETA, dev)


class _Bundle:
    def __init__(self, o, d, ln):
        self.origins, self.directions, self.lengths = o, d, ln


def test_autograd_route(cuda0):
    name = "H4 32-33 Wc40 C3"
    fld = _trainable(name, cuda0)
    frozen = fields.RadianceField(*gr.host_field(name)[1], dr.frequencies(4), gr.BETA, cuda0)
    o, d, ln, dd, dc = (_dev(a, cuda0) for a in _case(name, 43, 3))
    bundle = _Bundle(o.reshape(1, 43, 3), d.reshape(1, 43, 3), ln.reshape(1, 43, 3))
    dens, col = fld(bundle, cameras=None)
    fd, fc = frozen.forward(bundle)
    assert dens.shape == (1, 43, 3, 1) and col.shape == (1, 43, 3, 3) and dens.requires_grad and col.requires_grad
    assert torch.equal(dens.detach().view(torch.int32), fd.view(torch.int32))
    assert torch.equal(col.detach().view(torch.int32), fc.view(torch.int32))
    params = fld._params()
    shapes = ops.radiance_param_shapes(*gr.shape_args(name))

    def flat_grads():
        gW = torch.cat([p.grad.reshape(-1) for p in params[:len(shapes)]])
        gb = torch.cat([p.grad.reshape(-1) for p in params[len(shapes):]])
        for p in params:
            p.grad = None
        return gW.cpu().numpy(), gb.cpu().numpy()

    one_d, one_c = np.ones((43, 3), f32), np.ones((43, 3, 3), f32)
    (dens.sum() + col.sum()).backward()                                       # out.sum()
    got = flat_grads()
    want = _device_backward(name, cuda0, *_case(name, 43, 3)[:3], one_d, one_c)
    assert gr.same(got[0], want[0]) and gr.same(got[1], want[1])
    dens, col = fld.batched_forward(bundle, n_batches=4)
    (3 * ((dens[..., 0] * dd.reshape(1, 43, 3)).sum() + (col * dc.reshape(1, 43, 3, 3)).sum())).backward()      # 3 * f(out)
    got = flat_grads()
    want = _device_backward(name, cuda0, *_case(name, 43, 3)[:3], (3 * dd).cpu().numpy(), (3 * dc).cpu().numpy())
    assert gr.same(got[0], want[0]) and gr.same(got[1], want[1])
    dens, col = fld(bundle)
    col.sum().backward()                                                      # one output only used
    got = flat_grads()
    want = _device_backward(name, cuda0, *_case(name, 43, 3)[:3], None, one_c)
    assert gr.same(got[0], want[0]) and gr.same(got[1], want[1])
    with torch.no_grad():                                                     # a plain call
        dens, col = fld(bundle)
    assert not dens.requires_grad and torch.equal(dens.view(torch.int32), fd.view(torch.int32))
    with pytest.raises(NotImplementedError):
        fld(_Bundle(bundle.origins.clone().requires_grad_(True), bundle.directions, bundle.lengths))
    opt = torch.optim.SGD(fld.parameters(), lr=1e-2)                          # after a step: the new weights' forward
    dens, col = fld(bundle)
    (dens.sum() + col.sum()).backward()
    opt.step()
    with torch.no_grad():
        dens, col = fld(bundle)
    fresh = fld.to_radiance_field()
    fd2, fc2 = fresh.forward(bundle)
    assert torch.equal(dens.view(torch.int32), fd2.view(torch.int32)) and torch.equal(col.view(torch.int32), fc2.view(torch.int32))
    assert not torch.equal(fd2, fd)


def test_against_torch_on_the_device(cuda0):
    """The reference's widths at 4 097 points: every gradient array within PARITY_MARGIN x torch-f32's own deviation from
    torch-f64 (the same layers, same-arguments embedding, under autograd on the same device).  The yardstick is torch."""
    name = gr.REFERENCE
    _, w = gr.host_field(name)
    c = _case(name, 241, 17)
    ours = _device_backward(name, cuda0, *c)
    fr = dr.frequencies(60)
    r32 = gr.torch_grads(w, fr, gr.BETA, *c, torch.float32, cuda0)
    r64 = gr.torch_grads(w, fr, gr.BETA, *c, torch.float64, cuda0)
    entry, ok = {}, True
    for (k, mine), a32, a64 in zip(gr.split(name, *ours).items(), gr.split(name, *r32).values(), gr.split(name, *r64).values()):
        e = float(np.abs(a32 - a64).max())
        dev = float(np.abs(mine.astype(f64) - a64).max())
        print(f"{k}: deviation {dev:.3e}, torch f32 {e:.3e}, multiple {dev / e if e > 0 else float('nan'):.2f}")
        entry[k] = {"deviation": dev, "torch_f32": e, "multiple": dev / e if e > 0 else None}
        assert np.isfinite(e)
        ok = ok and dev <= (gr.PARITY_MARGIN * e if e > 0 else gr.ulp32(np.abs(a64).max()))
    gr.record("device vs torch on the device, 4 097 points", name, entry)
    assert ok, entry


def _scene(dev):
    """tests/test_gpu_ea_grad.py's scene: two cameras in front of the origin and 16 x 16 targets: a disc, coloured by position."""
    R = torch.eye(3)[None].repeat(2, 1, 1)
    R[1] = torch.tensor([[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]])
    cams = rays.PerspectiveCameras(R, torch.tensor([[0.0, 0.0, 2.5], [0.1, 0.0, 2.5]]), focal_length=2.0, in_ndc=True, device=dev)
    y, x = torch.meshgrid(torch.linspace(-1, 1, 16), torch.linspace(-1, 1, 16), indexing="ij")
    sil = ((x ** 2 + y ** 2) < 0.5).float()
    img = torch.stack([0.5 + 0.5 * x, 0.5 + 0.5 * y, 0.5 * torch.ones_like(x)], dim=-1) * sil[..., None]
    return cams, img[None].repeat(2, 1, 1, 1).to(dev), sil[None].repeat(2, 1, 1).to(dev)


def _five_steps(dev):
    mk = lambda seed: fields.TrainableRadianceField(*rr.fixture(4, 32, 1, 32, 3, seed=seed), dr.frequencies(4), 10.0, dev)
    coarse, fine = mk(3), mk(4)
    cams, images, silhouettes = _scene(dev)
    marcher = rays.EmissionAbsorptionRaymarcherStratified()
    sampler = rays.MonteCarloRaysampler(-1.0, 1.0, -1.0, 1.0, 32, 16, 1.0, 4.0, stratified_sampling=True, seed=7)
    r_coarse = rays.ImplicitRendererStratified(sampler, marcher, device=dev)
    r_fine = rays.ImplicitRendererStratified(sampler, marcher, device=dev, fine_seed=9)
    opt = torch.optim.Adam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-3)
    out, first_grads = [], None
    for _ in range(5):
        step = training.nerf_train_step(coarse, fine, r_coarse, r_fine, opt, cams, images, silhouettes)
        if first_grads is None:
            first_grads = [p.grad.detach().cpu().clone() for m in (coarse, fine) for p in m.parameters()]
        out.append(torch.stack([step["loss"], step["color_err"], step["sil_err"]]).cpu())
    return torch.stack(out), first_grads


def test_nerf_train_step_with_trainable_fields(cuda0):
    losses_a, grads = _five_steps(cuda0)
    print("losses of five steps:", [round(float(v), 4) for v in losses_a[:, 0]])
    assert len(grads) == 16 and all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads)      # every parameter, both fields
    assert torch.isfinite(losses_a).all()
    assert losses_a[4, 0] < losses_a[0, 0]                                            # five steps of Adam: the loss has fallen
    losses_b, _ = _five_steps(cuda0)                                                  # a fresh run: the same bytes
    assert poison.same_bits(losses_a, losses_b)
