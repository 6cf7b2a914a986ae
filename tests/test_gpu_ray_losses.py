"""GPU: the ray losses of include/isr_ray_losses.h.  The device entries against the host build of the same header (which
tests/test_ray_losses_cpu.py holds to the NumPy restatement and to the reference's executed code) bit for bit, at every count
around the kernels' widths; outputs and workspace written whatever they held, with guard bands; the autograd routes; the
gradient through the march; the memory a call needs; and training.nerf_train_step with both options."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import fields, losses, ops, rays, training
from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import ptr

from . import density_ref as dr
from . import ea_grad_ref as eg
from . import poison
from . import radiance_ref as rr
from . import ray_losses_ref as ref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DISTORTION = ref.distortion_cases()
RENDER = ref.render_cases()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _distortion_agrees(L, W, dev, upstreams=ref.UPSTREAMS):
    Ld, Wd = _dev(L, dev), _dev(W, dev)
    rays_h, loss_h = ops.distortion_forward_host(L, W)
    rays_d, loss_d = ops.distortion_forward(Ld, Wd)
    ok = ref.same(rays_d.cpu().numpy(), rays_h) and ref.same(loss_d.cpu().numpy(), loss_h)
    for up in upstreams:
        dw = ops.distortion_backward(Ld, Wd, torch.tensor([up], dtype=torch.float32, device=dev))
        ok = ok and ref.same(dw.cpu().numpy(), ops.distortion_backward_host(L, W, up))
    return ok


def _render_agrees(case, dev, upstreams=ref.RENDER_UPSTREAMS):
    on = [_dev(a, dev) for a in case]
    ok = ref.same(ops.render_loss_forward(*on).cpu().numpy(), ops.render_loss_forward_host(*case))
    for up in upstreams:
        g = ops.render_loss_backward(*on, torch.tensor(up, dtype=torch.float32, device=dev))
        ok = ok and ref.same(g.cpu().numpy(), ops.render_loss_backward_host(*case, up))
    return ok


def shape_cases():
    """N around the rays of a workgroup (4), a reduction tree (256) and two levels of trees (65 536), with a ragged last
    workgroup at 4 097; P at the limit."""
    rng = np.random.default_rng(77)
    geo = {"group_rays": 4, "reduce": 256}                # test_geometry holds them to the library
    counts = sorted({n for w in geo.values() for n in (w - 1, w, w + 1, 2 * w + 1)} | {4097})
    out = {f"N = {N}": (ref.fine_depths(rng, N, 20), ref.march_weights(rng, N, 20)) for N in counts}
    out["N = 65537, P = 3"] = (ref.fine_depths(rng, 65537, 3), ref.march_weights(rng, 65537, 3))
    out["N = 7, P = 1024"] = (ref.fine_depths(rng, 7, 1024), ref.march_weights(rng, 7, 1024, 0.05))
    return out


SHAPES = shape_cases()


def test_geometry(hip_lib):
    assert ops.ray_losses_geometry() == {"group_rays": 4, "lanes": 64, "reduce": 256, "max_p": 1024}


@pytest.mark.parametrize("name", list(DISTORTION))
def test_distortion_device_equals_host_on_the_cpu_cases(cuda0, name):
    assert _distortion_agrees(*DISTORTION[name], cuda0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_distortion_device_equals_host_at_the_shapes(cuda0, name):
    assert _distortion_agrees(*SHAPES[name], cuda0, upstreams=(-2.5,))


EDGES = ref.tree_edge_cases()


@pytest.mark.parametrize("name", list(EDGES))
def test_distortion_at_the_level_edges_of_the_ordered_sum(cuda0, name):
    """N = 1, 256, 257, 65 536 and 65 537 leaves (P = 2): the device, the host build and the f64 tree of
    tests/ray_losses_ref.py give the same bits below, at and above one tree of 256 and two levels of trees."""
    L, W = EDGES[name]
    want_rays, want_loss = ref.distortion_forward(L, W)
    rays_h, loss_h = ops.distortion_forward_host(L, W)
    rays_d, loss_d = ops.distortion_forward(_dev(L, cuda0), _dev(W, cuda0))
    rays_d, loss_d = rays_d.cpu().numpy(), loss_d.cpu().numpy()
    assert ref.same(rays_d, rays_h) and ref.same(loss_d, loss_h)
    assert ref.same(rays_d, want_rays) and ref.same(loss_d, want_loss)
    assert ref.same(rays_h, want_rays) and ref.same(loss_h, want_loss)


def test_a_row_alone_among_4097_and_beside_a_nan_row(cuda0):
    L, W = (a.copy() for a in SHAPES["N = 4097"])
    Ld, Wd = _dev(L, cuda0), _dev(W, cuda0)
    rays_all = ops.distortion_forward(Ld, Wd)[0].cpu().numpy()
    dw_all = ops.distortion_backward(Ld, Wd, torch.tensor([4097.0], device=cuda0)).cpu().numpy()      # c = upstream / N = 1
    one = torch.ones(1, device=cuda0)
    for i in (0, 2049, 4096):
        alone = ops.distortion_forward(Ld[i:i + 1], Wd[i:i + 1])[0].cpu().numpy()
        assert ref.same(alone, rays_all[i:i + 1])
        assert ref.same(ops.distortion_backward(Ld[i:i + 1], Wd[i:i + 1], one).cpu().numpy(), dw_all[i:i + 1])
    L[2049] = 2.5                                                                     # all depths equal: a NaN row
    Ld = _dev(L, cuda0)
    rays_nan, loss_nan = ops.distortion_forward(Ld, Wd)
    dw_nan = ops.distortion_backward(Ld, Wd, torch.tensor([4097.0], device=cuda0)).cpu().numpy()
    rays_nan, others = rays_nan.cpu().numpy(), np.arange(4097) != 2049
    assert np.isnan(rays_nan[2049]) and torch.isnan(loss_nan) and np.isnan(dw_nan[2049, :-1]).all()
    assert not dw_nan[:, -1].view(np.uint32).any()
    assert ref.same(rays_nan[others], rays_all[others]) and ref.same(dw_nan[others], dw_all[others])
    assert _distortion_agrees(L, W, cuda0, upstreams=(1.0,))


def render_shapes():
    rng = np.random.default_rng(78)
    out = {f"B n = {n}": ref.render_case(rng, 1, n, 3, 6, 6) for n in (255, 256, 257, 513)}
    out["B = 16, n = 1025"] = ref.render_case(rng, 16, 1025, 3, 32, 32)
    out["B n = 65537, F = 1"] = ref.render_case(rng, 1, 65537, 1, 5, 5)
    return out


RENDER_SHAPES = render_shapes()


@pytest.mark.parametrize("name", list(RENDER))
def test_render_loss_device_equals_host_on_the_cpu_cases(cuda0, name):
    assert _render_agrees(RENDER[name], cuda0)


@pytest.mark.parametrize("name", list(RENDER_SHAPES))
def test_render_loss_device_equals_host_at_the_shapes(cuda0, name):
    assert _render_agrees(RENDER_SHAPES[name], cuda0, upstreams=((-2.5, 3.0),))


# ---- outputs and workspace
GUARD = 256


def _banded(nbytes, byte, dev):
    """A buffer of nbytes filled with `byte` between two guard bands of the same byte -> (whole, its payload's address)."""
    whole = torch.full((GUARD + nbytes + GUARD,), byte, dtype=torch.uint8, device=dev)
    return whole, whole.data_ptr() + GUARD


def _payload(whole, byte):
    """The payload's bytes on the host, after checking that both guard bands still hold `byte`."""
    host = whole.cpu().numpy()
    assert (host[:GUARD] == byte).all() and (host[-GUARD:] == byte).all(), "a guard band was written"
    return host[GUARD:-GUARD]


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x7F])
def test_outputs_and_workspace_written_whatever_they_held(cuda0, byte):
    L, st = ops.lib(), torch.cuda.current_stream(cuda0).cuda_stream
    lengths, weights = SHAPES["N = 513"]
    N, P = lengths.shape
    Ld, Wd, up = _dev(lengths, cuda0), _dev(weights, cuda0), torch.tensor([-2.5], device=cuda0)
    want_rays, want_loss = ops.distortion_forward_host(lengths, weights)
    want_dw = ops.distortion_backward_host(lengths, weights, -2.5)
    ws_bytes = L.isr_distortion_workspace_bytes(N, P)
    assert 0 < ws_bytes <= 16 * N + 1024                                              # O(N), whatever P is
    assert L.isr_distortion_workspace_bytes(N, 1024) == ws_bytes
    ws, ws_p = _banded(ws_bytes, byte, cuda0)
    for with_rays in (True, False, True):                                             # ray_loss left out; the workspace reused
        rl, rl_p = _banded(4 * N, byte, cuda0)
        lo, lo_p = _banded(4, byte, cuda0)
        assert L.isr_distortion_forward(ptr(Ld), ptr(Wd), N, P, rl_p if with_rays else None, lo_p, ws_p, ws_bytes, st) == 0
        torch.cuda.synchronize()
        assert ref.same(_payload(lo, byte).view(f32), want_loss.reshape(1))
        got = _payload(rl, byte)
        assert ref.same(got.view(f32), want_rays) if with_rays else (got == byte).all()
        _payload(ws, byte)
    dw, dw_p = _banded(4 * N * P, byte, cuda0)
    assert L.isr_distortion_backward(ptr(Ld), ptr(Wd), N, P, ptr(up), dw_p, st) == 0
    torch.cuda.synchronize()
    assert ref.same(_payload(dw, byte).view(f32).reshape(N, P), want_dw)

    case = RENDER_SHAPES["B n = 513"]
    on = [_dev(a, cuda0) for a in case]
    B, n, F, H, W = 1, 513, 3, 6, 6
    up2 = torch.tensor([-2.5, 3.0], device=cuda0)
    ws_bytes = L.isr_render_loss_workspace_bytes(B, n)
    ws, ws_p = _banded(ws_bytes, byte, cuda0)
    for _ in range(2):
        out, out_p = _banded(8, byte, cuda0)
        assert L.isr_render_loss_forward(*map(ptr, on), B, n, F, H, W, 0.1, out_p, ws_p, ws_bytes, st) == 0
        torch.cuda.synchronize()
        assert ref.same(_payload(out, byte).view(f32), ops.render_loss_forward_host(*case))
        _payload(ws, byte)
    dr_, dr_p = _banded(4 * B * n * (F + 1), byte, cuda0)
    assert L.isr_render_loss_backward(*map(ptr, on), B, n, F, H, W, 0.1, ptr(up2), dr_p, st) == 0
    torch.cuda.synchronize()
    assert ref.same(_payload(dr_, byte).view(f32).reshape(B, n, F + 1), ops.render_loss_backward_host(*case, (-2.5, 3.0)))


def test_poisoned_allocations_a_second_call_and_a_callers_stream(cuda0, monkeypatch):
    lengths, weights = SHAPES["N = 4097"]
    Ld, Wd, up = _dev(lengths, cuda0), _dev(weights, cuda0), torch.tensor([1.0], device=cuda0)
    case = RENDER_SHAPES["B = 16, n = 1025"]
    on, up2 = [_dev(a, cuda0) for a in case], torch.tensor([1.0, 1.0], device=cuda0)

    def run():
        return (*ops.distortion_forward(Ld, Wd), ops.distortion_backward(Ld, Wd, up), ops.render_loss_forward(*on),
                ops.render_loss_backward(*on, up2))

    want = (*ops.distortion_forward_host(lengths, weights), ops.distortion_backward_host(lengths, weights, 1.0),
            ops.render_loss_forward_host(*case), ops.render_loss_backward_host(*case, (1.0, 1.0)))
    a, b = poison.run_twice(monkeypatch, run)                                         # 0xFF and 0x7F
    for got in (a, b):
        assert all(ref.same(g.numpy(), w) for g, w in zip(got, want))
    first, second = poison.to_host(run()), poison.to_host(run())                      # two calls: identical bytes
    assert poison.same_bits(first, second) and poison.same_bits(first, a)
    side = torch.cuda.Stream(cuda0)
    side.wait_stream(torch.cuda.current_stream(cuda0))
    with torch.cuda.stream(side):
        on_side = run()
    side.synchronize()
    assert poison.same_bits(poison.to_host(on_side), first)


def test_refusals(cuda0):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import IsrError
    L, st = ops.lib(), torch.cuda.current_stream(cuda0).cuda_stream
    x = torch.ones((3, 1025), device=cuda0)
    one = torch.ones(1, device=cuda0)
    for P in (1, 1025):
        with pytest.raises(IsrError, match="P outside"):
            ops.distortion_forward(x[:, :P].contiguous(), x[:, :P].contiguous())
        with pytest.raises(IsrError, match="P outside"):
            ops.distortion_backward(x[:, :P].contiguous(), x[:, :P].contiguous(), one)
    with pytest.raises(IsrError, match="N < 1"):
        ops.distortion_forward(x[:0, :5].contiguous(), x[:0, :5].contiguous())
    y = x[:, :5].contiguous()
    ws = torch.zeros(1 << 12, dtype=torch.uint8, device=cuda0)
    out = torch.full((8,), 7.0, device=cuda0)
    assert L.isr_distortion_forward(None, ptr(y), 3, 5, None, ptr(out), ptr(ws), ws.numel(), st) == -1
    assert L.isr_distortion_forward(ptr(y), None, 3, 5, None, ptr(out), ptr(ws), ws.numel(), st) == -1
    assert L.isr_distortion_forward(ptr(y), ptr(y), 3, 5, None, None, ptr(ws), ws.numel(), st) == -1
    assert L.isr_distortion_forward(ptr(y), ptr(y), 3, 5, None, ptr(out), None, ws.numel(), st) == -1
    assert L.isr_distortion_forward(ptr(y), ptr(y), 3, 5, None, ptr(out), ptr(ws), L.isr_distortion_workspace_bytes(3, 5) - 1, st) == -1
    assert b"workspace" in L.isr_last_error()
    assert L.isr_distortion_backward(ptr(y), ptr(y), 3, 5, None, ptr(out), st) == -1
    assert L.isr_distortion_backward(ptr(y), ptr(y), 3, 5, ptr(one), None, st) == -1
    assert L.isr_render_loss_forward(ptr(y), ptr(y), ptr(y), ptr(y), 1, 1, 1, 1, 1, 0.1, ptr(out), ptr(ws), 8, st) == -1
    assert L.isr_render_loss_forward(ptr(y), ptr(y), ptr(y), None, 1, 1, 1, 1, 1, 0.1, ptr(out), ptr(ws), ws.numel(), st) == -1
    assert L.isr_render_loss_backward(ptr(y), ptr(y), ptr(y), ptr(y), 1, 1, 1, 1, 1, 0.0, ptr(one), ptr(out), st) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                         # a refused call writes nothing


# ---- the autograd routes
def test_autograd_equals_the_entry(cuda0):
    lengths, weights = SHAPES["N = 257"]
    Ld = _dev(lengths.reshape(1, 257, 20), cuda0)
    Wd = _dev(weights.reshape(1, 257, 20), cuda0).requires_grad_(True)
    bundle = SimpleNamespace(lengths=Ld)
    loss = losses.mip360loss(bundle, Wd)
    assert loss.shape == () and ref.same(loss.detach().cpu().numpy(), ops.distortion_forward_host(lengths, weights)[1])
    loss.backward()
    assert Wd.grad.shape == Wd.shape and ref.same(Wd.grad.cpu().numpy().reshape(257, 20), ops.distortion_backward_host(lengths, weights, 1.0))
    Wd.grad = None
    (3 * losses.mip360loss(bundle, Wd)).backward()
    assert ref.same(Wd.grad.cpu().numpy().reshape(257, 20), ops.distortion_backward_host(lengths, weights, 3.0))
    with pytest.raises(NotImplementedError):
        losses.mip360loss(SimpleNamespace(lengths=Ld.clone().requires_grad_(True)), Wd)
    W64 = Wd.detach().double().transpose(0, 1).requires_grad_(True)                   # not f32, not contiguous: converted
    losses.distortion_loss(Ld.transpose(0, 1), W64).backward()
    assert W64.grad.dtype == torch.float64 and ref.same(W64.grad.float().cpu().numpy().reshape(257, 20),
                                                        ops.distortion_backward_host(lengths, weights, 1.0))
    case = RENDER["F = 3"]
    on = [_dev(a, cuda0) for a in case]
    x = on[0].clone().requires_grad_(True)
    col, sil = losses.render_loss(x, *on[1:])
    assert ref.same(torch.stack([col, sil]).detach().cpu().numpy(), ops.render_loss_forward_host(*case))
    (col - 2.5 * sil).backward()
    assert ref.same(x.grad.cpu().numpy(), ops.render_loss_backward_host(*case, (1.0, -2.5)))


def test_through_the_march(cuda0):
    """densities.grad of images.sum() + mip360loss(bundle, weights) is ops.ea_march_backward fed the entry's dweights, bit for
    bit, and lies within 4 x torch-f32's own deviation from the same expression in torch f64 on the device."""
    rng = np.random.default_rng(5)
    N, P, F = 65, 33, 3
    rho, feat = eg.densities(rng, "small", N, P), rng.standard_normal((N, P, F)).astype(f32)
    lengths = _dev(ref.fine_depths(rng, N, P), cuda0)
    d, f = _dev(rho.reshape(N, P, 1), cuda0).requires_grad_(True), _dev(feat, cuda0)
    images, weights = rays.EmissionAbsorptionRaymarcherStratified()(d, f)
    (images.sum() + losses.mip360loss(SimpleNamespace(lengths=lengths), weights)).backward()
    dweights = ops.distortion_backward(lengths, weights.detach(), torch.ones(1, device=cuda0))
    want = ops.ea_march_backward(d.detach().reshape(N, P), f, torch.ones((N, F + 1), device=cuda0), dweights, need=(True, False))[0]
    assert ref.same(d.grad.reshape(N, P).cpu().numpy(), want.cpu().numpy())
    grads = {}
    for dtype in (torch.float32, torch.float64):
        dt = d.detach().to(dtype).reshape(N, P).requires_grad_(True)
        im, wt = eg.pren_march(dt, f.to(dtype))
        (im.sum() + ref.torch_formula(lengths.to(dtype), wt)).backward()
        grads[dtype] = dt.grad.double().cpu().numpy()
    e = float(np.abs(grads[torch.float32] - grads[torch.float64]).max())
    dev = float(np.abs(d.grad.reshape(N, P).double().cpu().numpy() - grads[torch.float64]).max())
    print(f"through the march: deviation {dev:.3e}, torch f32 {e:.3e}, multiple {dev / e:.2f}")
    ref.record("device through the march against torch f64 on the device", {"ddensities": round(dev / e, 3)})
    assert e > 0 and dev <= ref.PARITY_MARGIN * e


def test_memory_does_not_grow_with_p(cuda0):
    """Peak allocation beyond the inputs and dweights is the same at P = 64 and P = 512: nothing per pair is stored."""
    rng = np.random.default_rng(6)
    extra = {}
    for P in (64, 512, 64):                                                           # the first round warms the cached workspace
        Ld = _dev(ref.fine_depths(rng, 2048, P), cuda0)
        Wd, one = _dev(ref.march_weights(rng, 2048, P), cuda0), torch.ones(1, device=cuda0)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()                                                      # no cached block of another size to hand out
        torch.cuda.reset_peak_memory_stats(cuda0)
        base = torch.cuda.memory_allocated(cuda0)
        ops.distortion_forward(Ld, Wd, want_ray_loss=False)
        dweights = ops.distortion_backward(Ld, Wd, one)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated(cuda0) - base                               # dweights, as the allocator rounds it
        extra[P] = torch.cuda.max_memory_allocated(cuda0) - base - held
        assert held >= dweights.numel() * 4
        del dweights                                                                  # not inside the next round's window
    print("peak bytes beyond the inputs and dweights:", extra)
    assert extra[64] == extra[512] and extra[64] < (1 << 16)


# ---- the training step
def _scene(dev):
    """Two cameras in front of the origin and 8 x 8 targets: a disc, coloured by position."""
    R = torch.eye(3)[None].repeat(2, 1, 1)
    R[1] = torch.tensor([[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]])
    cams = rays.PerspectiveCameras(R, torch.tensor([[0.0, 0.0, 2.5], [0.1, 0.0, 2.5]]), focal_length=2.0, in_ndc=True, device=dev)
    y, x = torch.meshgrid(torch.linspace(-1, 1, 8), torch.linspace(-1, 1, 8), indexing="ij")
    sil = ((x ** 2 + y ** 2) < 0.5).float()
    img = torch.stack([0.5 + 0.5 * x, 0.5 + 0.5 * y, 0.5 * torch.ones_like(x)], dim=-1) * sil[..., None]
    return cams, img[None].repeat(2, 1, 1, 1).to(dev), sil[None].repeat(2, 1, 1).to(dev)


def _steps(dev, count, **options):
    """`count` steps of two fresh small TrainableRadianceFields -> (losses (count, 3 or 4), the first step's gradients)."""
    mk = lambda seed: fields.TrainableRadianceField(*rr.fixture(4, 32, 1, 32, 3, seed=seed), dr.frequencies(4), 10.0, dev)
    coarse, fine = mk(3), mk(4)
    cams, images, silhouettes = _scene(dev)
    marcher = rays.EmissionAbsorptionRaymarcherStratified()
    sampler = rays.MonteCarloRaysampler(-1.0, 1.0, -1.0, 1.0, 32, 16, 1.0, 4.0, stratified_sampling=True, seed=7)
    r_coarse = rays.ImplicitRendererStratified(sampler, marcher, device=dev)
    r_fine = rays.ImplicitRendererStratified(sampler, marcher, device=dev, fine_seed=9)
    opt = torch.optim.Adam(list(coarse.parameters()) + list(fine.parameters()), lr=5e-3)
    out, first_grads = [], None
    for _ in range(count):
        step = training.nerf_train_step(coarse, fine, r_coarse, r_fine, opt, cams, images, silhouettes, **options)
        if first_grads is None:
            first_grads = [p.grad.detach().cpu().clone() for m in (coarse, fine) for p in m.parameters()]
        out.append(torch.stack([step[k] for k in ("loss", "color_err", "sil_err", "distortion") if k in step]).cpu())
    return torch.stack(out), first_grads


def _parent_step(coarse_field, fine_field, renderer_coarse, renderer_fine, optimizer, cameras, target_images, target_silhouettes):
    """The step as it stood before the options: the same calls into the package, statement by statement."""
    optimizer.zero_grad()
    rendered, sampled_rays, weights = renderer_coarse(cameras=cameras, volumetric_function=coarse_field, add_input_samples=False,
                                                      stratified=False)
    rendered_fine, sampled_rays2, _ = renderer_fine(cameras=cameras, volumetric_function=fine_field, add_input_samples=True,
                                                    stratified=True, coarse=(sampled_rays, weights.detach()))
    xys = sampled_rays2.xys
    last = rendered.shape[-1]
    images, silhouettes = rendered.split([last - 1, 1], dim=-1)
    images_fine, silhouettes_fine = rendered_fine.split([last - 1, 1], dim=-1)
    silhouettes_at_rays = rays.sample_images_at_mc_locs(target_silhouettes[..., None], xys)
    colors_at_rays = rays.sample_images_at_mc_locs(target_images, xys)
    sil_err = losses.huber(silhouettes, silhouettes_at_rays).abs().mean()
    color_err = losses.huber(images, colors_at_rays).abs().mean()
    sil_err = sil_err + losses.huber(silhouettes_fine, silhouettes_at_rays).abs().mean()
    color_err = color_err + losses.huber(images_fine, colors_at_rays).abs().mean()
    sil_err, color_err = 500 * sil_err, 500 * color_err
    loss = color_err + sil_err
    loss.backward()
    optimizer.step()
    return {"loss": loss.detach(), "color_err": color_err.detach(), "sil_err": sil_err.detach()}


def test_the_default_step_is_the_parents(cuda0, monkeypatch):
    """Called without the new arguments the step gives the bytes of the step as it stood, five steps long."""
    plain, grads = _steps(cuda0, 5)
    monkeypatch.setattr(training, "nerf_train_step", _parent_step)
    parent, parent_grads = _steps(cuda0, 5)
    assert plain.shape == (5, 3) and poison.same_bits(plain, parent) and poison.same_bits(grads, parent_grads)


def test_fused_losses_in_the_step(cuda0):
    """color_err and sil_err of the first step with fused_losses=True against the default route.  Both routes round the same
    exact value: the default one carries torch-f32's own deviation, which the fixture measures as a fraction of the loss
    (render_out_eref / render_out_f64), the fused one at most PARITY_MARGIN times that (tests/test_ray_losses_cpu.py), and the sum of
    the two renders and the factor 500 round once each on either route: half an f32 ulp each, 2 ulp in all."""
    fx = ref.fixture()
    plain, _ = _steps(cuda0, 1)
    fused, grads = _steps(cuda0, 1, fused_losses=True)
    assert len(grads) == 16 and all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads)
    for col, v in ((1, 0), (2, 1)):
        a, b = float(plain[0, col]), float(fused[0, col])
        rel = float(fx["render_out_eref"][v] / fx["render_out_f64"][v])
        bound = (1 + ref.PARITY_MARGIN) * rel * abs(a) + 2 * ref.ulp32(a)
        print(f"{('color_err', 'sil_err')[v]}: default {a!r}, fused {b!r}, difference {abs(a - b):.3e}, bound {bound:.3e}")
        assert abs(a - b) <= bound
    assert abs(float(fused[0, 0]) - float(fused[0, 1]) - float(fused[0, 2])) <= ref.ulp32(fused[0, 0])


def test_distortion_in_the_step_and_both_options_twice(cuda0):
    with_d, grads = _steps(cuda0, 1, distortion_weight=0.01)
    assert with_d.shape == (1, 4) and torch.isfinite(with_d).all() and with_d[0, 3] > 0
    assert len(grads) == 16 and all(torch.isfinite(g).all() for g in grads)
    plain, plain_grads = _steps(cuda0, 1)
    assert poison.same_bits(with_d[0, 1:3], plain[0, 1:3])                            # the same render: the same Huber terms
    assert any(not torch.equal(g, h) for g, h in zip(grads, plain_grads))             # and the regulariser reaches the fields
    a, _ = _steps(cuda0, 5, distortion_weight=0.01, fused_losses=True)
    b, _ = _steps(cuda0, 5, distortion_weight=0.01, fused_losses=True)
    assert a.shape == (5, 4) and torch.isfinite(a).all() and poison.same_bits(a, b)
