"""GPU: isr_sample_nearest_backward against the host build of the same header (which tests/test_sample_grad_cpu.py holds to
the NumPy restatement of include/isr_sample_grad.h), bit for bit with NaN-aware equality, on both sort paths and at their
seams; every output written whatever the buffers held; and the autograd route of rays.sample_images_at_mc_locs."""
import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import losses, ops, rays
from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import ptr

from . import poison
from . import rays_ref as rr
from . import sample_grad_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = ref.cases()
LDS, BLOCK = 4096, 1024                                # isr_sample_grad_geometry(0), (1): test_geometry holds them to the library


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device(case, dev):
    dout, xys, H, W = case
    return ops.sample_at_rays_backward(_dev(dout, dev), _dev(xys, dev), H, W).cpu().numpy()


def _agrees(case, dev):
    dout, xys, H, W = case
    return ref.same_bits(_device(case, dev), ops.sample_at_rays_backward_host(dout, xys, H, W))


def seam_cases():
    """n one below, at and one above the LDS path's limit, the radix block and a block boundary of the radix path, all
    rays on one pixel and random; images past one and two radix digits; a segment across a radix block boundary; the
    channel counts around a wave."""
    rng = np.random.default_rng(77)
    out = {}
    for n in (LDS - 1, LDS, LDS + 1, BLOCK - 1, BLOCK, BLOCK + 1, LDS + BLOCK - 1, LDS + BLOCK, LDS + BLOCK + 1):
        out[f"one pixel, n = {n}"] = ref.one_pixel_case(rng, 2, 5, 7, 2, n)
        out[f"random, n = {n}"] = ref.random_case(rng, 2, 9, 11, 2, n)
    out["3 x 100 pixels, radix"] = ref.random_case(rng, 2, 3, 100, 1, LDS + 900)
    out["300 x 300 pixels, radix"] = ref.random_case(rng, 2, 300, 300, 1, LDS + 900)
    out["300 x 300 pixels, LDS"] = ref.random_case(rng, 2, 300, 300, 1, 700)
    n = LDS + 904
    iy = np.where(np.arange(n) < BLOCK - 24, 1, np.where(np.arange(n) < BLOCK + 76, 2, 3))      # pixel (2, 0): positions 1000 .. 1099
    out["a segment across a radix block boundary"] = (rng.standard_normal((1, n, 3)).astype(f32),
                                                     ref.on_pixels(iy, np.zeros(n), 5, 4)[None], 5, 4)
    for C in (63, 64, 65):
        out[f"C = {C}"] = ref.random_case(rng, 2, 6, 7, C, 130)
    out["224 x 224, every ray on its own pixel"] = (rng.standard_normal((1, 224 * 224, 1)).astype(f32),
                                                   rr.grid_xys(224, 224).reshape(1, -1, 2), 224, 224)
    return out


SEAMS = seam_cases()


def test_geometry(hip_lib):
    assert ops.sample_grad_geometry() == {"lds_rays": LDS, "block_keys": BLOCK, "digit_bits": 8}


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_on_the_cpu_cases(cuda0, name):
    assert _agrees(CASES[name], cuda0)


@pytest.mark.parametrize("name", list(SEAMS))
def test_device_equals_host_at_the_seams(cuda0, name):
    assert _agrees(SEAMS[name], cuda0)


def test_the_full_grid_is_a_permutation(cuda0):
    dout, xys, H, W = SEAMS["224 x 224, every ray on its own pixel"]
    got = _device((dout, xys, H, W), cuda0)
    assert ref.same_bits(got.reshape(-1), dout.reshape(-1) + f32(0))                  # ray r is pixel r; -0 + 0 = +0


@pytest.mark.parametrize("name", ["C = 13", "B = 3, the middle image keeps nothing", "random, n = 5121", "300 x 300 pixels, radix"])
def test_outputs_and_workspace_written_whatever_they_held(cuda0, monkeypatch, name):
    case = {**CASES, **SEAMS}[name]
    dout, xys, H, W = case
    want = ops.sample_at_rays_backward_host(dout, xys, H, W)
    d, x = _dev(dout, cuda0), _dev(xys, cuda0)
    a, b = poison.run_twice(monkeypatch, lambda: ops.sample_at_rays_backward(d, x, H, W))      # 0xFF and 0x7F
    assert ref.same_bits(a.numpy(), want) and ref.same_bits(b.numpy(), want)
    L, st = ops.lib(), torch.cuda.current_stream(cuda0).cuda_stream
    B, n, C = dout.shape
    nb = L.isr_sample_grad_workspace_bytes(B, H, W, n)
    for byte in (0x00, 0xFF):
        ws = torch.full((nb,), byte, dtype=torch.uint8, device=cuda0)
        res = torch.empty((B, H, W, C), dtype=torch.float32, device=cuda0)
        res.view(torch.uint8).fill_(byte)
        assert L.isr_sample_nearest_backward(ptr(d), B, H, W, C, ptr(x), n, ptr(res), ptr(ws), nb, st) == 0
        assert ref.same_bits(res.cpu().numpy(), want)


def test_middle_image_keeps_nothing(cuda0):
    got = _device(CASES["B = 3, the middle image keeps nothing"], cuda0)
    assert not got[1].view(np.uint32).any() and got[0].any() and got[2].any()


def test_reused_workspace_second_call_and_a_callers_stream(cuda0):
    ops.clear_workspaces()
    large, small = SEAMS["random, n = 5121"], CASES["C = 12"]
    first = _device(small, cuda0)
    assert _agrees(large, cuda0)                                                      # grows the cached workspace
    again = _device(small, cuda0)                                                     # the smaller call in the larger buffer
    assert ref.same_bits(first, again) and ref.same_bits(again, ops.sample_at_rays_backward_host(*small))
    assert ref.same_bits(_device(large, cuda0), _device(large, cuda0))                # two calls, equal bytes
    side = torch.cuda.Stream(cuda0)
    side.wait_stream(torch.cuda.current_stream(cuda0))
    with torch.cuda.stream(side):
        on_side = [ops.sample_at_rays_backward(_dev(c[0], cuda0), _dev(c[1], cuda0), c[2], c[3]) for c in (small, large)]
    side.synchronize()
    for got, case in zip(on_side, (small, large)):
        assert ref.same_bits(got.cpu().numpy(), ops.sample_at_rays_backward_host(*case))
    ops.clear_workspaces()


def test_unaligned_output(cuda0):
    """dimages 4 bytes past a 16-byte boundary: the fill's head, body and tail."""
    dout, xys, H, W = CASES["C = 13"]
    B, n, C = dout.shape
    L, st = ops.lib(), torch.cuda.current_stream(cuda0).cuda_stream
    nb = L.isr_sample_grad_workspace_bytes(B, H, W, n)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda0)
    total = B * H * W * C
    buf = torch.full((total + 8,), float("nan"), dtype=torch.float32, device=cuda0)
    d, x = _dev(dout, cuda0), _dev(xys, cuda0)
    assert L.isr_sample_nearest_backward(ptr(d), B, H, W, C, ptr(x), n, ptr(buf) + 4, ptr(ws), nb, st) == 0
    host = buf.cpu().numpy()
    assert ref.same_bits(host[1:1 + total].reshape(B, H, W, C), ops.sample_at_rays_backward_host(dout, xys, H, W))
    assert np.isnan(host[0]) and np.isnan(host[1 + total:]).all()                     # nothing written outside


# ---- autograd through rays.sample_images_at_mc_locs
def _collide(rng, B, H, W, C, n):
    """Rays drawn so that some pixels are hit more than once."""
    feat = rng.standard_normal((B, H, W, C)).astype(f32)
    xys = rng.uniform(-1.05, 1.05, (B, n, 2)).astype(f32)
    return feat, xys


def test_feat_grad_equals_the_entry(cuda0):
    rng = np.random.default_rng(3)
    feat_h, xys_h = _collide(rng, 2, 6, 7, 12, 200)
    xys = _dev(xys_h, cuda0)
    feat = _dev(feat_h, cuda0).requires_grad_(True)
    out = rays.sample_images_at_mc_locs(feat, xys)
    assert out.grad_fn is not None and torch.equal(out.detach(), ops.sample_at_rays(feat.detach(), xys))
    out.sum().backward()
    assert ref.same_bits(feat.grad.cpu().numpy(), ops.sample_at_rays_backward_host(np.ones((2, 200, 12), f32), xys_h, 6, 7))
    feat.grad = None
    w = _dev(rng.standard_normal((2, 200, 12)).astype(f32), cuda0)
    out = rays.sample_images_at_mc_locs(feat, xys)
    (3 * (out * w).sum()).backward()
    dout = 3 * w                                                                      # one rounding, as autograd makes it
    assert ref.same_bits(feat.grad.cpu().numpy(), ops.sample_at_rays_backward(dout, xys, 6, 7).cpu().numpy())


def test_feat_grad_against_grid_sample_in_f64_on_the_device(cuda0):
    rng = np.random.default_rng(4)
    feat_h, xys_h = _collide(rng, 2, 6, 7, 5, 300)
    w_h = rng.standard_normal((2, 300, 5)).astype(f32)
    feat = _dev(feat_h, cuda0).requires_grad_(True)
    (rays.sample_images_at_mc_locs(feat, _dev(xys_h, cuda0)) * _dev(w_h, cuda0)).sum().backward()
    f64 = _dev(feat_h, cuda0).double().requires_grad_(True)
    smp = torch.nn.functional.grid_sample(f64.permute(0, 3, 1, 2), -_dev(xys_h, cuda0).double().view(2, -1, 1, 2), align_corners=True,
                                          mode="nearest")
    (smp.permute(0, 2, 3, 1).view(2, 300, 5) * _dev(w_h, cuda0).double()).sum().backward()
    _, a, m = ref.sums_f64(w_h, xys_h, 6, 7)
    assert m.max() > 1
    # torch's f64 atomics add in any order: their own rounding, m * 2^-53 * sum|dout|, is far below one f32 ulp of the bound
    err = np.abs(feat.grad.cpu().numpy().astype(np.float64) - f64.grad.cpu().numpy())
    assert np.all(err <= ref.chain_bound(a, m) + m[..., None] * 2.0 ** -53 * a)
    single = np.broadcast_to((m <= 1)[..., None], err.shape)
    assert not err[single].any()


def test_sliced_input_and_xys_grad(cuda0):
    """trainPose.py's own input: movedim(...)[..., 0:12] of a 13-channel NCHW tensor; the 13th channel gets exactly 0."""
    rng = np.random.default_rng(6)
    nchw = _dev(rng.standard_normal((2, 13, 6, 7)).astype(f32), cuda0).requires_grad_(True)
    xys_h = rng.uniform(-1.05, 1.05, (2, 150, 2)).astype(f32)
    xys = _dev(xys_h, cuda0).requires_grad_(True)
    feat12 = torch.movedim(nchw, 1, 3)[..., 0:12]
    assert not feat12.is_contiguous()
    w = _dev(rng.standard_normal((2, 150, 12)).astype(f32), cuda0)
    (rays.sample_images_at_mc_locs(feat12, xys) * w).sum().backward()
    g = torch.movedim(nchw.grad, 1, 3).cpu().numpy()
    assert not g[..., 12].view(np.uint32).any()
    assert ref.same_bits(np.ascontiguousarray(g[..., :12]), ops.sample_at_rays_backward_host(w.cpu().numpy(), xys_h, 6, 7))
    assert xys.grad is not None and xys.grad.shape == xys.shape and not xys.grad.cpu().numpy().view(np.uint32).any()


@pytest.mark.parametrize("shape", [(2, 6, 9, 12, 300), (1, 224, 224, 3, 1000), (3, 5, 1, 1, 17), (2, 4, 5, 65, 64)])
def test_without_a_gradient_the_plain_route(cuda0, shape):
    B, H, W, C, n = shape
    rng = np.random.default_rng(sum(shape))
    feat, xys = _dev(rng.standard_normal((B, H, W, C)).astype(f32), cuda0), _dev(rng.uniform(-1.1, 1.1, (B, n, 2)).astype(f32), cuda0)
    out = rays.sample_images_at_mc_locs(feat, xys)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, ops.sample_at_rays(feat, xys))
    with torch.no_grad():
        quiet = rays.sample_images_at_mc_locs(feat.clone().requires_grad_(True), xys)
    assert quiet.grad_fn is None and torch.equal(quiet, out)
    tracked = rays.sample_images_at_mc_locs(feat.clone().requires_grad_(True), xys)
    assert tracked.grad_fn is not None and torch.equal(tracked.detach(), out)         # the same bits either way


def test_the_loss_reaches_the_encoder_output(cuda0):
    """returnCrossEntropyWithNeg(sample_images_at_mc_locs(feat, xys), k, neg).backward() gives feat a gradient."""
    rng = np.random.default_rng(8)
    feat = _dev(rng.standard_normal((2, 8, 8, 12)).astype(f32), cuda0).requires_grad_(True)
    xys = _dev(rng.uniform(-1, 1, (2, 64, 2)).astype(f32), cuda0)
    k, neg = _dev(rng.standard_normal((2, 64, 12)).astype(f32), cuda0), _dev(rng.standard_normal((2, 64, 12)).astype(f32), cuda0)
    losses.returnCrossEntropyWithNeg(rays.sample_images_at_mc_locs(feat, xys), k, neg).backward()
    assert feat.grad is not None and torch.isfinite(feat.grad).all() and feat.grad.abs().sum() > 0
