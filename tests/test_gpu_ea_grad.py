"""GPU: isr_ea_march_backward against the host build of the same header (which tests/test_ea_grad_cpu.py holds to the NumPy
restatement of include/isr_ea_grad.h), bit for bit with NaN-aware equality, at every count around the rays a workgroup owns;
every output written whatever the buffers held; the autograd route of rays.EmissionAbsorptionRaymarcherStratified; and one
training.nerf_train_step."""
import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops, rays, training
from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import ptr

from . import ea_grad_ref as ref
from . import poison

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = ref.cases()
GROUP = {1: 64, 64: 63, 128: 31, 256: 15, 2048: 1}     # isr_ea_grad_rays_per_group(P): test_geometry holds them to the library


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _device(case, dev, need=(True, True)):
    rho, feat, dimage, dw, thr = case
    out = ops.ea_march_backward(_dev(rho, dev), _dev(feat, dev), _dev(dimage, dev), _dev(dw, dev), thr, need)
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def _host(case, need=(True, True)):
    rho, feat, dimage, dw, thr = case
    return ops.ea_march_backward_host(rho, feat, dimage, dw, thr, need)


def _agrees(case, dev):
    got, want = _device(case, dev), _host(case)
    return ref.same_bits(got[0], want[0]) and ref.same_bits(got[1], want[1])


def shape_cases():
    """N around a wave, a workgroup's threads and past one grid of pairs; P at the issue's sizes and F at the channel counts,
    at a small N; and every ray count around a workgroup's share, at each P whose share differs."""
    rng = np.random.default_rng(99)
    out = {}
    for N in (1, 63, 64, 65, 257, 4097):
        out[f"N = {N}"] = ref.random_case(rng, N, 9, 3, "small")
    for P in (1, 2, 64, 65, 128, 257, 1024):
        out[f"P = {P}"] = ref.random_case(rng, 7, P, 3, ("uniform", "small", "sharp")[P % 3])
    for F in (1, 3, 12, 16, 17, 33):
        out[f"F = {F}"] = ref.random_case(rng, 70, 33, F, "small")
    for P, R in GROUP.items():
        for N in sorted({max(R - 1, 1), R, R + 1, 2 * R, 2 * R + 1}):
            out[f"P = {P}, {R} rays a workgroup, N = {N}"] = ref.random_case(rng, N, P, 3, "small", threshold=0.04 if N == R + 1 else -1.0)
    out["P = 4096, F = 64"] = ref.random_case(rng, 3, 4096, 64, "small", dweights=False)
    return out


SHAPES = shape_cases()


def test_geometry(hip_lib):
    assert {P: ops.ea_grad_rays_per_group(P) for P in GROUP} == GROUP
    assert ops.ea_grad_geometry() == {"threads": 256, "max_group_rays": 64, "row_floats": 4097}


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_on_the_cpu_cases(cuda0, name):
    assert _agrees(CASES[name], cuda0)


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_host_at_the_shapes(cuda0, name):
    assert _agrees(SHAPES[name], cuda0)


@pytest.mark.parametrize("name", ["P = 65, F = 17", "one NaN ray among clean rays", "threshold mode, 0.02", "P = 64, 63 rays a workgroup, N = 127"])
def test_outputs_written_whatever_they_held(cuda0, monkeypatch, name):
    case = {**CASES, **SHAPES}[name]
    want = _host(case)
    dev_case = tuple(_dev(a, cuda0) for a in case[:4])
    a, b = poison.run_twice(monkeypatch, lambda: ops.ea_march_backward(*dev_case, case[4]))      # 0xFF and 0x7F
    for got in (a, b):
        assert ref.same_bits(got[0].numpy(), want[0]) and ref.same_bits(got[1].numpy(), want[1])
    L, st = ops.lib(), torch.cuda.current_stream(cuda0).cuda_stream
    N, P, F = case[1].shape
    for byte in (0x00, 0x7F, 0xFF):                                                   # through the C ABI, and each output null
        dd, df = (torch.full(s, byte, dtype=torch.uint8, device=cuda0) for s in ((N, P, 4), (N, P, F, 4)))
        for outs in ((dd, df), (dd, None), (None, df)):
            for o in outs:
                if o is not None:
                    o.fill_(byte)
            assert L.isr_ea_march_backward(ptr(dev_case[0]), ptr(dev_case[1]), N, P, F, case[4], ptr(dev_case[2]), ptr(dev_case[3]),
                                           ptr(outs[0]), ptr(outs[1]), st) == 0
            for o, w in zip(outs, want):
                assert o is None or ref.same_bits(o.cpu().numpy().view(f32).reshape(w.shape), w)


def test_each_output_alone_a_second_call_and_a_callers_stream(cuda0):
    small, large = CASES["P = 64, F = 3"], SHAPES["N = 4097"]
    for case in (small, large):
        want = _host(case)
        only_dd, none = _device(case, cuda0, (True, False))
        assert none is None and ref.same_bits(only_dd, want[0])
        none, only_df = _device(case, cuda0, (False, True))
        assert none is None and ref.same_bits(only_df, want[1])
    first = _device(small, cuda0)
    assert _agrees(large, cuda0)
    again = _device(small, cuda0)                                                     # a second call: nothing is left behind
    assert ref.same_bits(first[0], again[0]) and ref.same_bits(first[1], again[1])
    a, b = _device(large, cuda0), _device(large, cuda0)                               # two calls, equal bytes
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    side = torch.cuda.Stream(cuda0)
    side.wait_stream(torch.cuda.current_stream(cuda0))
    with torch.cuda.stream(side):
        on_side = [ops.ea_march_backward(*(_dev(x, cuda0) for x in c[:4]), c[4]) for c in (small, large)]
    side.synchronize()
    for got, case in zip(on_side, (small, large)):
        want = _host(case)
        assert ref.same_bits(got[0].cpu().numpy(), want[0]) and ref.same_bits(got[1].cpu().numpy(), want[1])


def test_no_rays(cuda0):
    dd, df = ops.ea_march_backward(torch.zeros((0, 5), device=cuda0), torch.zeros((0, 5, 3), device=cuda0), torch.zeros((0, 4), device=cuda0))
    assert dd.shape == (0, 5) and df.shape == (0, 5, 3)


# ---- autograd through rays.EmissionAbsorptionRaymarcherStratified
def _inputs(rng, lead, P, F, dev, kind="small"):
    N = int(np.prod(lead))
    rho, feat = ref.densities(rng, kind, N, P), rng.standard_normal((N, P, F)).astype(f32)
    return rho, feat, _dev(rho.reshape(*lead, P, 1), dev), _dev(feat.reshape(*lead, P, F), dev)


def test_grads_equal_the_entry(cuda0):
    rng = np.random.default_rng(3)
    lead, P, F = (2, 35), 33, 3
    rho, feat, d, f = _inputs(rng, lead, P, F, cuda0)
    d.requires_grad_(True), f.requires_grad_(True)
    marcher = rays.EmissionAbsorptionRaymarcherStratified()
    images, weights = marcher(d, f)
    assert images.grad_fn is not None and weights.grad_fn is not None and images.shape == (*lead, F + 1) and weights.shape == (*lead, P)
    plain = ops.ea_march(d.detach().reshape(-1, P), f.detach().reshape(-1, P, F))
    assert torch.equal(images.detach().reshape(-1, F + 1), plain[0]) and torch.equal(weights.detach().reshape(-1, P), plain[1])
    images.sum().backward()                                                           # the weights unused: a null dweights
    want = ops.ea_march_backward_host(rho, feat, np.ones((70, F + 1), f32), None)
    assert d.grad.shape == d.shape and f.grad.shape == f.shape
    assert ref.same_bits(d.grad.cpu().numpy().reshape(70, P), want[0]) and ref.same_bits(f.grad.cpu().numpy().reshape(70, P, F), want[1])
    d.grad = f.grad = None
    wi = _dev(rng.standard_normal((*lead, F + 1)).astype(f32), cuda0)
    images, weights = marcher(d, f)
    (3 * (images * wi).sum() + weights.sum()).backward()
    want = ops.ea_march_backward((d.detach().reshape(-1, P)), f.detach().reshape(-1, P, F), (3 * wi).reshape(-1, F + 1),
                                 torch.ones((70, P), device=cuda0))                   # 3 * wi: one rounding, as autograd makes it
    assert ref.same_bits(d.grad.cpu().numpy().reshape(70, P), want[0].cpu().numpy())
    assert ref.same_bits(f.grad.cpu().numpy().reshape(70, P, F), want[1].cpu().numpy())
    d.grad = f.grad = None
    marcher(d, f)[1].sum().backward()                                                 # the images unused: dimage of zeros
    want = ops.ea_march_backward_host(rho, feat, np.zeros((70, F + 1), f32), np.ones((70, P), f32))
    assert ref.same_bits(d.grad.cpu().numpy().reshape(70, P), want[0]) and not f.grad.cpu().numpy().any()


def test_one_input_requiring_a_gradient_other_dtypes_and_threshold_mode(cuda0):
    rng = np.random.default_rng(4)
    rho, feat, d, f = _inputs(rng, (40,), 20, 5, cuda0)
    marcher = rays.EmissionAbsorptionRaymarcherStratified()
    want = ops.ea_march_backward_host(rho, feat, np.ones((40, 6), f32), None)
    dg = d.clone().requires_grad_(True)
    marcher(dg, f)[0].sum().backward()
    assert ref.same_bits(dg.grad.cpu().numpy().reshape(40, 20), want[0])
    fg = f.clone().requires_grad_(True)
    marcher(d, fg)[0].sum().backward()
    assert ref.same_bits(fg.grad.cpu().numpy(), want[1])
    d64 = d.double().requires_grad_(True)                                             # cast as the plain route casts: the gradient
    images, _ = marcher(d64, f)                                                       # returns in the input's dtype and shape
    images.sum().backward()
    assert images.dtype == torch.float32 and d64.grad.dtype == torch.float64 and d64.grad.shape == (40, 20, 1)
    assert ref.same_bits(d64.grad.float().cpu().numpy().reshape(40, 20), want[0])
    hard = rays.EmissionAbsorptionRaymarcherStratified(thresholdMode=True, threshold=0.02)
    dg.grad = None
    fg.grad = None
    images, weights = hard(dg, fg)
    assert torch.equal(images.detach(), ops.ea_march(d.reshape(40, 20), f, 0.02)[0])
    (images.sum() + weights.sum()).backward()
    want = ops.ea_march_backward_host(rho, feat, np.ones((40, 6), f32), np.ones((40, 20), f32), 0.02)
    assert not dg.grad.cpu().numpy().view(np.uint32).any() and ref.same_bits(fg.grad.cpu().numpy(), want[1])


@pytest.mark.parametrize("tag", ref.FIXTURES)
def test_against_the_expression_in_f64_on_the_device(cuda0, tag):
    """pren.py's formula in torch f64 on the device, on the fixture's inputs, within the CPU test's bound."""
    fx = ref.fixture(tag)
    N, P, F = fx["feat"].shape
    d, f = _dev(fx["rho"].reshape(N, P, 1), cuda0).requires_grad_(True), _dev(fx["feat"], cuda0).requires_grad_(True)
    wi, ww = _dev(fx["Wi"], cuda0), _dev(fx["Ww"], cuda0)
    images, weights = rays.EmissionAbsorptionRaymarcherStratified()(d, f)
    ((images * wi).sum() + (weights * ww).sum()).backward()
    d64, f64 = d.detach().double().reshape(N, P).requires_grad_(True), f.detach().double().requires_grad_(True)
    images64, weights64 = ref.pren_march(d64, f64)
    ((images64 * wi.double()).sum() + (weights64 * ww.double()).sum()).backward()
    for name, got, want, E in (("ddensities", d.grad.reshape(N, P), d64.grad, fx["E_dd"]), ("dfeatures", f.grad, f64.grad, fx["E_df"])):
        want = want.cpu().numpy()
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print(f"{tag} {name}: err {err:.3e} = {err / E:.2f} x E_ref; bound {ref.bound(E, want):.3e}")
        assert err <= ref.bound(E, want)


@pytest.mark.parametrize("lead,P,F", [((2, 35), 33, 3), ((1200,), 64, 3), ((3, 5, 7), 1, 12)])
def test_without_a_gradient_the_plain_route(cuda0, lead, P, F):
    rng = np.random.default_rng(P)
    _, _, d, f = _inputs(rng, lead, P, F, cuda0)
    marcher = rays.EmissionAbsorptionRaymarcherStratified()
    images, weights = marcher(d, f)
    plain = ops.ea_march(d.reshape(-1, P), f.reshape(-1, P, F))
    assert images.grad_fn is None and weights.grad_fn is None and not images.requires_grad
    assert torch.equal(images.reshape(-1, F + 1), plain[0]) and torch.equal(weights.reshape(-1, P), plain[1])
    with torch.no_grad():
        quiet = marcher(d.clone().requires_grad_(True), f.clone().requires_grad_(True))
    assert quiet[0].grad_fn is None and quiet[1].grad_fn is None and torch.equal(quiet[0], images) and torch.equal(quiet[1], weights)
    tracked = marcher(d.clone().requires_grad_(True), f)
    assert tracked[0].grad_fn is not None and torch.equal(tracked[0].detach(), images) and torch.equal(tracked[1].detach(), weights)


def test_the_renderers_generic_route_and_its_coarse_weights_carry_gradients(cuda0):
    cams, _, _, _ = _scene(cuda0)
    field = _Field().to(cuda0)
    sampler = rays.MonteCarloRaysampler(-1.0, 1.0, -1.0, 1.0, 32, 16, 1.0, 4.0, seed=5)
    renderer = rays.ImplicitRendererStratified(sampler, rays.EmissionAbsorptionRaymarcherStratified(), device=cuda0, fine_seed=2)
    images, bundle, weights = renderer(cameras=cams, volumetric_function=field)
    assert images.grad_fn is not None and weights.grad_fn is not None and images.shape == (2, 32, 4)
    coarse = renderer._coarse_weights(bundle, cams, field, {})
    assert coarse.grad_fn is not None and torch.equal(coarse.detach(), weights.detach())
    images, fine, _ = renderer(cameras=cams, volumetric_function=field, stratified=True, add_input_samples=True)
    assert fine.lengths.shape == (2, 32, 32) and not fine.lengths.requires_grad
    images.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in field.parameters())


# ---- one step of trainNerfFine.py
class _Field(torch.nn.Module):
    """A harmonic embedding, Linear(.., 32) + Softplus, and the two heads of nerf.py's field: 1 - exp(-softplus) and a sigmoid."""

    def __init__(self, n_harmonic: int = 4, hidden: int = 32, F: int = 3):
        super().__init__()
        self.register_buffer("frequencies", 0.5 * 2.0 ** torch.arange(n_harmonic))
        self.trunk = torch.nn.Sequential(torch.nn.Linear(6 * n_harmonic, hidden), torch.nn.Softplus(beta=10.0))
        self.density = torch.nn.Sequential(torch.nn.Linear(hidden, 1), torch.nn.Softplus(beta=10.0))
        self.colour = torch.nn.Sequential(torch.nn.Linear(hidden, F), torch.nn.Sigmoid())

    def forward(self, ray_bundle, cameras=None, **kwargs):
        points = ray_bundle.origins[..., None, :] + ray_bundle.lengths[..., :, None] * ray_bundle.directions[..., None, :]
        e = (points[..., None] * self.frequencies).flatten(-2)
        h = self.trunk(torch.cat((e.sin(), e.cos()), dim=-1))
        return 1 - (-self.density(h)).exp(), self.colour(h)


def _scene(dev):
    """Two cameras in front of the origin and 16 x 16 targets: a disc, coloured by position."""
    R = torch.eye(3)[None].repeat(2, 1, 1)
    R[1] = torch.tensor([[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]])
    cams = rays.PerspectiveCameras(R, torch.tensor([[0.0, 0.0, 2.5], [0.1, 0.0, 2.5]]), focal_length=2.0, in_ndc=True, device=dev)
    y, x = torch.meshgrid(torch.linspace(-1, 1, 16), torch.linspace(-1, 1, 16), indexing="ij")
    sil = ((x ** 2 + y ** 2) < 0.5).float()
    img = torch.stack([0.5 + 0.5 * x, 0.5 + 0.5 * y, 0.5 * torch.ones_like(x)], dim=-1) * sil[..., None]
    return cams, img[None].repeat(2, 1, 1, 1).to(dev), sil[None].repeat(2, 1, 1).to(dev), None


def _five_steps(dev):
    torch.manual_seed(11)
    coarse, fine = _Field().to(dev), _Field().to(dev)
    cams, images, silhouettes, _ = _scene(dev)
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


def test_nerf_train_step(cuda0):
    losses_a, grads = _five_steps(cuda0)
    assert len(grads) == 12 and all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads)      # every parameter, both fields
    assert torch.isfinite(losses_a).all() and torch.allclose(losses_a[:, 0], losses_a[:, 1] + losses_a[:, 2])
    assert losses_a[4, 0] < losses_a[0, 0]                                            # five steps of Adam: the loss has fallen
    losses_b, _ = _five_steps(cuda0)                                                  # a fresh run: the same bytes
    assert poison.same_bits(losses_a, losses_b)
