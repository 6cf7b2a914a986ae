"""CPU: the host build of csrc/sample_grad.hpp (isr_sample_nearest_backward_host) against the NumPy restatement of
include/isr_sample_grad.h (tests/sample_grad_ref.py), bit for bit; against torch's grid_sample under autograd in f64 within
the first-order bound of the f32 chain, (m - 1) * 2^-24 * sum|dout| per entry (m the pixel's ray count), which is derived,
not measured; and the refusals of the C entries."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops

from . import sample_grad_ref as ref

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
CASES = ref.cases()


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def torch_grad_f64(dout, xys, H, W):
    """d sum(dout * grid_sample(images, -xys, nearest, align_corners=True)) / d images in f64, (B, H, W, C)."""
    B, n, C = dout.shape
    images = torch.zeros((B, H, W, C), dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.grid_sample(images.permute(0, 3, 1, 2), -torch.from_numpy(xys).double().view(B, n, 1, 2),
                                          align_corners=True, mode="nearest")
    out.backward(torch.from_numpy(dout).double().permute(0, 2, 1).reshape(B, C, n, 1))
    return images.grad.numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_host_equals_the_restatement(hip_lib, name):
    dout, xys, H, W = CASES[name]
    got = ops.sample_at_rays_backward_host(dout, xys, H, W)
    assert ref.same_bits(got, ref.backward_ref(dout, xys, H, W))
    _, _, m = ref.sums_f64(dout, xys, H, W)
    untouched = got[m == 0]
    assert not untouched.view(np.uint32).any()                                        # +0, not -0


def test_a_single_minus_zero_gives_plus_zero(hip_lib):
    got = ops.sample_at_rays_backward_host(np.full((1, 1, 2), -0.0, f32), np.zeros((1, 1, 2), f32), 3, 3)
    assert not got.view(np.uint32).any()


def test_nan_and_infinity_reach_only_their_entries(hip_lib):
    dout, xys, H, W = CASES["dout with a NaN and an infinity"]
    got = ops.sample_at_rays_backward_host(dout, xys, H, W)
    ix, iy = ref.nearest_pixel(xys[..., 0], W), ref.nearest_pixel(xys[..., 1], H)
    want = np.zeros(got.shape, bool)
    for b, r, c in ((0, 7, 1), (1, 11, 2)):
        assert ix[b, r] >= 0 and iy[b, r] >= 0                                        # the case puts both inside
        want[b, iy[b, r], ix[b, r], c] = True
    assert np.array_equal(~np.isfinite(got), want)


@pytest.mark.parametrize("name", [k for k in CASES if "NaN and an infinity" not in k])
def test_within_the_chain_bound_of_torch_f64(hip_lib, name):
    dout, xys, H, W = CASES[name]
    got = ops.sample_at_rays_backward_host(dout, xys, H, W).astype(np.float64)
    want = torch_grad_f64(dout, xys, H, W)
    s, a, m = ref.sums_f64(dout, xys, H, W)
    assert np.array_equal(want, s)                                                    # torch's f64 route is the f64 sum itself
    bound = ref.chain_bound(a, m)
    err = np.abs(got - want)
    used = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    print(f"{name}: worst entry uses {100 * used:.2f} % of its bound")
    assert np.all(err <= bound)
    single = np.broadcast_to((m <= 1)[..., None], got.shape)
    assert np.array_equal(got[single], want[single])


def test_one_image_on_one_pixel_among_two(hip_lib):
    """B = 2, 5 x 7 x 3, n = 4 097, image 0's rays all on one pixel, image 1's spread."""
    rng = np.random.default_rng(5)
    dout, xys, H, W = ref.random_case(rng, 2, 5, 7, 3, 4097)
    xys[0] = ref.on_pixels([2], [3], H, W)
    got = ops.sample_at_rays_backward_host(dout, xys, H, W)
    assert ref.same_bits(got, ref.backward_ref(dout, xys, H, W))
    s, a, m = ref.sums_f64(dout, xys, H, W)
    assert m[0, 2, 3] == 4097 and np.all(np.abs(got - s) <= ref.chain_bound(a, m))


def test_refusals(hip_lib):
    L = hip_lib
    dout, xys, res = np.zeros((2, 5, 3), f32), np.zeros((2, 5, 2), f32), np.zeros((2, 4, 4, 3), f32)
    nb = L.isr_sample_grad_workspace_bytes(2, 4, 4, 5)
    assert nb > 0
    ws = np.zeros(nb, np.uint8)
    for hole in range(3):
        a = [vp(dout), vp(xys), vp(res)]
        a[hole] = None
        assert L.isr_sample_nearest_backward_host(a[0], 2, 4, 4, 3, a[1], 5, a[2]) == -1 and b"null" in L.isr_last_error()
        assert L.isr_sample_nearest_backward(a[0], 2, 4, 4, 3, a[1], 5, a[2], vp(ws), nb, None) == -1 and b"null" in L.isr_last_error()
    assert L.isr_sample_nearest_backward(vp(dout), 2, 4, 4, 3, vp(xys), 5, vp(res), None, nb, None) == -1
    assert L.isr_sample_nearest_backward(vp(dout), 2, 4, 4, 3, vp(xys), 5, vp(res), vp(ws), nb - 1, None) == -1
    assert b"workspace" in L.isr_last_error()
    for B, H, W, C, n, word in ((0, 4, 4, 3, 5, b"B"), (2, 0, 4, 3, 5, b"H"), (2, 4, 0, 3, 5, b"W"), (2, 4, 4, 0, 5, b"C"),
                                (2, 4, 4, 4097, 5, b"C"), (2, 4, 4, 3, 0, b"n"), (2, 4, 4, 3, (1 << 27) + 1, b"2^28"),
                                (2, 4, 4, 4096, 1 << 18, b"2^31"), (1, 1 << 16, 1 << 15, 3, 5, b"2^31 - 1"),
                                (1 << 12, 1 << 14, 1 << 14, 1, 5, b"2^40"), (1, 1 << 14, 1 << 14, 4096, 5, b"2^40")):
        assert L.isr_sample_nearest_backward_host(vp(dout), B, H, W, C, vp(xys), n, vp(res)) == -1 and word in L.isr_last_error()
        assert L.isr_sample_nearest_backward(vp(dout), B, H, W, C, vp(xys), n, vp(res), vp(ws), nb, None) == -1
        assert word in L.isr_last_error()
    for B, H, W, n in ((0, 4, 4, 5), (2, 4, 4, 0), (1 << 14, 4, 4, (1 << 14) + 1), (1, 1 << 16, 1 << 15, 5)):
        assert L.isr_sample_grad_workspace_bytes(B, H, W, n) == 0 and L.isr_last_error()
    for call in (lambda: ops.sample_at_rays_backward_host(dout[0], xys, 4, 4), lambda: ops.sample_at_rays_backward_host(dout, xys[:1], 4, 4),
                 lambda: ops.sample_at_rays_backward_host(dout, xys[..., :1], 4, 4), lambda: ops.sample_at_rays_backward_host(dout, xys, 0, 4),
                 lambda: ops.sample_at_rays_backward_host(np.zeros((2, 5, 4097), f32), xys, 4, 4)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_capi.IsrError):
        ops.sample_at_rays_backward(torch.from_numpy(dout), torch.from_numpy(xys), 4, 4)                  # no CPU fall-back


def test_workspace_grows_with_the_path(hip_lib):
    L, g = hip_lib, ops.sample_grad_geometry()
    assert g == {"lds_rays": 4096, "block_keys": 1024, "digit_bits": 8} and L.isr_sample_grad_geometry(3) == -1
    small, large = L.isr_sample_grad_workspace_bytes(2, 224, 224, g["lds_rays"]), L.isr_sample_grad_workspace_bytes(2, 224, 224, g["lds_rays"] + 1)
    assert small >= 2 * 2 * g["lds_rays"] * 4 and large >= 2 * small
    assert L.isr_sample_grad_workspace_bytes(2, 3, 3, 100) == L.isr_sample_grad_workspace_bytes(2, 300, 300, 100)


def test_header_and_signature_table(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_sample_grad.h").read_text(), flags=re.S)
    decls = {m.group(1): m.group(2) for m in re.finditer(r"\b(isr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}
    assert sorted(decls) == sorted(_capi.SAMPLE_GRAD_SIGNATURES) and len(decls) == 4
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_sample_grad.h but not exported"
        assert len(_capi.SAMPLE_GRAD_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    main = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_hip.h").read_text(), flags=re.S)
    assert "isr_sample" not in main and hip_lib.isr_abi_version() == 6


def test_the_autograd_route_refuses_cpu_tensors_and_leaves_the_plain_route_alone(hip_lib):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import rays
    img, xy = torch.zeros((2, 3, 3, 2), requires_grad=True), torch.zeros((2, 5, 2))
    with pytest.raises(_capi.IsrError):
        rays.sample_images_at_mc_locs(img, xy)
    with pytest.raises(_capi.IsrError):
        rays.sample_images_at_mc_locs(img.detach(), xy)
