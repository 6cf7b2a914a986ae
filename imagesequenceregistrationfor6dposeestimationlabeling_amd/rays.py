"""Rays from cameras on the device, under pytorch3d's names: PerspectiveCameras, NDCMultinomialRaysampler,
MonteCarloRaysampler and RayBundle as generateCors.py:125-138, :279-293 and genFeat.py:102-106, :162-189 use them, and the
silhouette selection of pren.py:229-236 (`sampler(cameras, mask=...)`).  The rays come from the isr_rays_* entries
(include/isr_rays.h states every rule, and which of them are pytorch3d's only as far as they are known from memory); this
module holds the camera's bookkeeping and the conversion of screen-space intrinsics to NDC.  On top of them the renderer
of pren.py under its names: EmissionAbsorptionRaymarcherStratified (pren.py:256-369) and ImplicitRendererStratified
(pren.py:172-253), whose images come from isr_ea_march or, for a fields.RadianceField, from the fused isr_radiance_render.
The fine pass's depths — sample_pdf and ProbabilisticRaysampler (pren.py:372-457), the renderer's stratified=True — come from
isr_resample_lengths (include/isr_resample.h; the rule of sample_pdf is pytorch3d's only as far as it is known from memory).

Out of scope: the raymarcher's weightMode, unit_directions, K= and FoV cameras."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .ops import RAYS_GRID, RAYS_MC, RaySpec


class RayBundle(NamedTuple):
    origins: torch.Tensor       # (..., 3)
    directions: torch.Tensor    # (..., 3), not normalised: origins + directions * z is the point at camera depth z
    lengths: torch.Tensor       # (..., P)
    xys: torch.Tensor           # (..., 2) NDC, +x left, +y up


def _rows(name: str, v, B: int, device, per_camera: bool = False) -> torch.Tensor:
    """v as a (B, 2) f32 tensor.  A scalar, (B, 1) and (B, 2) broadcast; a 1-D value is one per camera when per_camera
    (focal_length (B,)), otherwise one row (2,)."""
    t = torch.as_tensor(v).to(device=device, dtype=torch.float32)
    if t.ndim == 0:
        t = t.reshape(1, 1)
    elif t.ndim == 1:
        t = t.reshape(-1, 1) if per_camera else t.reshape(1, -1)
    if t.ndim != 2 or t.shape[0] not in (1, B) or t.shape[1] not in (1, 2) or (t.shape[1] == 1 and not (per_camera or t.shape[0] == 1)):
        raise ValueError(f"PerspectiveCameras: {name} must broadcast to ({B},2), got {tuple(torch.as_tensor(v).shape)}")
    return t.expand(B, 2).contiguous()


class PerspectiveCameras:
    """Row-vector cameras: X_cam = X_world R + T, x_ndc = fx X/Z + px; NDC is +x left, +y up.

    R (B,3,3), T (B,3); focal_length (B,) or (B,2) and principal_point (B,2) in pixels unless in_ndc, image_size (H, W) (or
    (B,2) rows of it).  With in_ndc=False the intrinsics are mapped to NDC with s = min(H, W):
        f_ndc = f * 2 / s,   px_ndc = -(px - W/2) * 2 / s,   py_ndc = -(py - H/2) * 2 / s
    — pytorch3d's documented formula AS FAR AS IT IS KNOWN FROM MEMORY (unpinned: pytorch3d is not available); the signs are
    held by tests/test_rays_cpu.py to BOP poses converted as in generateCors.py:98-102 and their OpenCV pixels.
    cameras[idx] (an int, a slice, a list or a tensor of indices) and len(cameras) work as in pytorch3d."""

    def __init__(self, R, T, focal_length=1.0, principal_point=((0.0, 0.0),), image_size=None, in_ndc: bool = False, device=None,
                 K=None):
        if K is not None:
            raise ValueError("PerspectiveCameras: K= is not supported; give focal_length and principal_point")
        R = torch.as_tensor(R)
        device = torch.device(device) if device is not None else R.device
        self.R = R.to(device=device, dtype=torch.float32).contiguous()
        self.T = torch.as_tensor(T).to(device=device, dtype=torch.float32).contiguous()
        if self.R.ndim != 3 or tuple(self.R.shape[1:]) != (3, 3) or self.R.shape[0] < 1 or tuple(self.T.shape) != (self.R.shape[0], 3):
            raise ValueError(f"PerspectiveCameras: R must be (B,3,3) and T (B,3), got {tuple(self.R.shape)} and {tuple(self.T.shape)}")
        B = self.R.shape[0]
        f = _rows("focal_length", focal_length, B, device, per_camera=True)
        p = _rows("principal_point", principal_point, B, device)
        self.in_ndc = bool(in_ndc)
        self.image_size = None
        if not self.in_ndc:
            if image_size is None:
                raise ValueError("PerspectiveCameras: screen-space intrinsics (in_ndc=False) need image_size = (H, W)")
            hw = _rows("image_size", image_size, B, device)
            if not bool((hw >= 1).all()):
                raise ValueError("PerspectiveCameras: image_size must be at least 1 x 1")
            self.image_size = hw
            s = hw.min(dim=1, keepdim=True).values
            wh = hw.flip(1)                                          # (W, H) beside (px, py)
            f = f * 2 / s
            p = -(p - wh / 2) * 2 / s
        self.intrinsics = torch.cat([f, p], dim=1).contiguous()      # (B, 4): fx, fy, px, py in NDC
        self.device = device

    def __len__(self) -> int:
        return self.R.shape[0]

    def __getitem__(self, idx) -> "PerspectiveCameras":
        if isinstance(idx, int):
            idx = [idx]
        if not isinstance(idx, slice):
            idx = torch.as_tensor(idx, device=self.device)
            if idx.dtype == torch.bool or idx.ndim != 1:
                raise IndexError("PerspectiveCameras: index with an int, a slice or a 1-D list / tensor of indices")
            idx = idx.long()
        out = object.__new__(PerspectiveCameras)
        out.R, out.T, out.intrinsics = self.R[idx].contiguous(), self.T[idx].contiguous(), self.intrinsics[idx].contiguous()
        out.image_size = None if self.image_size is None else self.image_size[idx].contiguous()
        out.in_ndc, out.device = self.in_ndc, self.device
        if len(out) < 1:
            raise IndexError("PerspectiveCameras: the index selects no camera")
        return out

    def to(self, device) -> "PerspectiveCameras":
        out = object.__new__(PerspectiveCameras)
        out.device = torch.device(device)
        out.R, out.T, out.intrinsics = self.R.to(out.device), self.T.to(out.device), self.intrinsics.to(out.device)
        out.image_size = None if self.image_size is None else self.image_size.to(out.device)
        out.in_ndc = self.in_ndc
        return out


def _bundle(spec: RaySpec, cameras: PerspectiveCameras, mask, camera_ids, host: bool, shape) -> RayBundle:
    """The bundle of `spec`: every ray reshaped to (B, *shape, .) without a mask, the kept rays as (1, M, .) with one."""
    if not isinstance(cameras, PerspectiveCameras):
        raise TypeError("a raysampler takes rays.PerspectiveCameras")
    cams = (cameras.R, cameras.T, cameras.intrinsics)
    if host:
        cams = tuple(c.cpu().numpy() for c in cams)
        ids = None if camera_ids is None else np.asarray(torch.as_tensor(camera_ids).cpu())
        if mask is None:
            o, d, ln, xy = (torch.from_numpy(a) for a in ops.rays_bundle_host(spec, *cams, ids))
        else:
            o, d, ln, xy = (torch.from_numpy(a) for a in ops.rays_select_host(spec, *cams, torch.as_tensor(mask).cpu().numpy(), ids)[:4])
    else:
        ids = None if camera_ids is None else torch.as_tensor(camera_ids, device=cameras.device)
        if mask is None:
            o, d, ln, xy = ops.rays_bundle(spec, *cams, ids)
        else:
            o, d, ln, xy = ops.rays_select(spec, *cams, torch.as_tensor(mask).to(cameras.device), ids)[:4]
    if mask is not None:
        return RayBundle(o[None], d[None], ln[None], xy[None])
    B = len(cameras)
    return RayBundle(o.reshape(B, *shape, 3), d.reshape(B, *shape, 3), ln.reshape(B, *shape, spec.P), xy.reshape(B, *shape, 2))


class NDCMultinomialRaysampler:
    """One ray through the centre of every pixel of an image_height x image_width grid, in raster order, with n_pts_per_ray
    depths linspace(min_depth, max_depth) (generateCors.py:136, genFeat.py:102).

    sampler(cameras) -> RayBundle of (B, H, W, .) on the cameras' device.
    sampler(cameras, mask=(B, mh, mw[, 1])) -> the (1, M, .) bundle of pren.py:232-235: the rays whose xy falls on a non-zero
    pixel of their camera's mask, in (camera, ray) order; one host read, of the count.
    camera_ids is accepted for the samplers' common call and not read: a grid ray does not depend on it."""

    def __init__(self, image_width: int, image_height: int, n_pts_per_ray: int, min_depth: float, max_depth: float):
        self.spec = RaySpec(RAYS_GRID, int(n_pts_per_ray), float(min_depth), float(max_depth), W=int(image_width), H=int(image_height))

    def __call__(self, cameras: PerspectiveCameras, mask=None, camera_ids=None, host: bool = False) -> RayBundle:
        return _bundle(self.spec, cameras, mask, None, host, (self.spec.H, self.spec.W))


class MonteCarloRaysampler:
    """n_rays_per_image rays per camera at uniform NDC locations in [min_x, max_x) x [min_y, max_y) (generateCors.py:138,
    genFeat.py:105), from Philox4x32-10 under `seed`: torch's random stream is not reproduced.  camera_ids (B,) names the
    cameras (default 0 .. B-1): a ray is a function of (seed, camera_id, ray index) only, so a camera draws the same rays
    alone and inside a batch.  A caller who wants fresh rays per call (genFeat.py's 19 rounds) changes the seed.
    stratified_sampling moves every depth inside its stratum (include/isr_rays.h).

    sampler(cameras) -> RayBundle of (B, n, .); sampler(cameras, mask=...) -> (1, M, .) as for the grid sampler."""

    def __init__(self, min_x: float, max_x: float, min_y: float, max_y: float, n_rays_per_image: int, n_pts_per_ray: int,
                 min_depth: float, max_depth: float, stratified_sampling: bool = False, seed: int = 0):
        self.spec = RaySpec(RAYS_MC, int(n_pts_per_ray), float(min_depth), float(max_depth), n=int(n_rays_per_image),
                            min_x=float(min_x), max_x=float(max_x), min_y=float(min_y), max_y=float(max_y),
                            stratified=bool(stratified_sampling), seed=int(seed))

    def __call__(self, cameras: PerspectiveCameras, mask=None, camera_ids=None, host: bool = False) -> RayBundle:
        return _bundle(self.spec, cameras, mask, camera_ids, host, (self.spec.n,))


def sample_images_at_mc_locs(target_images: torch.Tensor, sampled_rays_xy: torch.Tensor) -> torch.Tensor:
    """nutil.sample_images_at_mc_locs (nutil.py:167-196): target_images (B,H,W,C) at the NDC locations (B,...,2) -> (B,...,C),
    the nearest pixel of -xy with zeros outside, on the device (ops.sample_at_rays).
    When gradients are enabled and target_images requires one, the result carries it back (trainPose.py:397-400 trains the
    encoder through this call): the values are the same bits, and the backward is ops.sample_at_rays_backward, per pixel the
    f32 sum of its rays in ray order with no float atomics (include/isr_sample_grad.h), once differentiable.  A
    non-contiguous or non-f32 target_images is copied by a torch op first, which carries the gradient on to the original.
    sampled_rays_xy, if it requires a gradient, gets zeros, as torch's nearest-mode grid_sample gives it."""
    if torch.is_grad_enabled() and target_images.requires_grad:
        return _SampleAtRays.apply(ops._f32c(target_images), sampled_rays_xy)
    return ops.sample_at_rays(target_images, sampled_rays_xy)


class _SampleAtRays(torch.autograd.Function):
    """images (B,H,W,C) f32 contiguous, xys (B,...,2) -> (B,...,C): ops.sample_at_rays forward, ops.sample_at_rays_backward
    backward.  Only xys and the image size are saved."""

    @staticmethod
    def forward(ctx, images, xys):
        out = ops.sample_at_rays(images.detach(), xys.detach())
        ctx.save_for_backward(xys.detach())
        ctx.size = (int(images.shape[1]), int(images.shape[2]))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        xys, = ctx.saved_tensors
        dimages = ops.sample_at_rays_backward(dout.contiguous(), xys, *ctx.size) if ctx.needs_input_grad[0] else None
        return dimages, torch.zeros_like(xys) if ctx.needs_input_grad[1] else None


def sample_pdf(bins: torch.Tensor, weights: torch.Tensor, n_samples: int, det: bool = False, eps: float = 1e-5, *,
               seed: int = 0) -> torch.Tensor:
    """pytorch3d's sample_pdf: bins (..., nb+1), weights (..., nb) -> samples (..., n_samples) by inverse-CDF sampling, on
    the device (ops.sample_pdf; include/isr_resample.h states the rule).  det: evenly spaced units, otherwise Philox under
    `seed` with the flattened row index as the ray id — torch's random stream is not reproduced."""
    lead = tuple(bins.shape[:-1])
    if tuple(weights.shape[:-1]) != lead:
        raise ValueError(f"sample_pdf: bins {tuple(bins.shape)} and weights {tuple(weights.shape)} differ in their leading shape")
    out = ops.sample_pdf(bins.to(torch.float32).reshape(-1, bins.shape[-1]).contiguous(),
                         weights.to(torch.float32).reshape(-1, weights.shape[-1]).contiguous(), n_samples, det, eps, seed)
    return out.reshape(*lead, int(n_samples))


class ProbabilisticRaysampler:
    """pren.py:372-457: sampler(input_ray_bundle, ray_weights) -> the RayBundle whose lengths are n_pts_per_ray depths drawn
    from the coarse ray_weights (..., P), together with the input lengths when add_input_samples, sorted; origins, directions
    and xys are passed through.  Any leading shape is taken, so the view() calls of pren.py:216-224 are not needed.
    The units are evenly spaced unless (stratified and training) or (stratified_test and not training), when they come from
    Philox under `seed` with the flattened ray index as the ray id; a caller who wants fresh samples changes `seed`."""

    def __init__(self, n_pts_per_ray: int, stratified: bool, stratified_test: bool, add_input_samples: bool = True, seed: int = 0):
        self._n_pts_per_ray = int(n_pts_per_ray)
        self._stratified = bool(stratified)
        self._stratified_test = bool(stratified_test)
        self._add_input_samples = bool(add_input_samples)
        self.seed = int(seed)
        self.training = True

    def train(self, mode: bool = True) -> "ProbabilisticRaysampler":
        self.training = bool(mode)
        return self

    def eval(self) -> "ProbabilisticRaysampler":
        return self.train(False)

    def __call__(self, input_ray_bundle: RayBundle, ray_weights: torch.Tensor, **kwargs) -> RayBundle:
        z = input_ray_bundle.lengths
        if tuple(ray_weights.shape) != tuple(z.shape):
            raise ValueError(f"ProbabilisticRaysampler: ray_weights {tuple(ray_weights.shape)} for lengths {tuple(z.shape)}")
        det = not ((self._stratified and self.training) or (self._stratified_test and not self.training))
        P = z.shape[-1]
        out = ops.resample_lengths(z.to(torch.float32).reshape(-1, P).contiguous(),
                                   ray_weights.to(torch.float32).reshape(-1, P).contiguous(), self._n_pts_per_ray,
                                   self._add_input_samples, det, seed=self.seed)
        return RayBundle(input_ray_bundle.origins, input_ray_bundle.directions, out.reshape(*z.shape[:-1], out.shape[-1]),
                         input_ray_bundle.xys)

    forward = __call__


def ea_march(rays_densities: torch.Tensor, rays_features: torch.Tensor, threshold: float = -1.0):
    """rays_densities (..., P, 1) and rays_features (..., P, F) -> (images (..., F+1) [features | opacity], weights (..., P))
    by ops.ea_march; threshold >= 0 is thresholdMode.  Inputs that are not f32 are cast first.
    When gradients are enabled and an input requires one, the results carry it back (trainNerfFine.py:353 trains the fields
    through this call): the values are the same bits, and the backward is ops.ea_march_backward, per ray an adjoint
    recurrence with no division and no float atomics (include/isr_ea_grad.h), once differentiable.  The casts and reshapes
    are torch ops, so a gradient arrives in its input's dtype and shape.  In thresholdMode the densities get zeros."""
    lead, P, F = tuple(rays_features.shape[:-2]), rays_features.shape[-2], rays_features.shape[-1]
    dens, feat = rays_densities.to(torch.float32).reshape(-1, P), rays_features.to(torch.float32).reshape(-1, P, F)
    if torch.is_grad_enabled() and (dens.requires_grad or feat.requires_grad):
        image, wts = _EaMarch.apply(dens, feat, float(threshold))
    else:
        image, wts = ops.ea_march(dens.contiguous(), feat.contiguous(), threshold, want_weights=True)
    return image.reshape(*lead, F + 1), wts.reshape(*lead, P)


class _EaMarch(torch.autograd.Function):
    """densities (N,P), features (N,P,F) f32 -> image (N,F+1), weights (N,P): ops.ea_march forward, ops.ea_march_backward
    backward.  An output nobody used arrives as None: a null dweights, or zeros for dimage."""

    @staticmethod
    def forward(ctx, densities, features, threshold):
        dens, feat = densities.detach().contiguous(), features.detach().contiguous()
        image, wts = ops.ea_march(dens, feat, threshold, want_weights=True)
        ctx.save_for_backward(dens, feat)
        ctx.threshold = threshold
        ctx.set_materialize_grads(False)
        return image, wts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dimage, dweights):
        dens, feat = ctx.saved_tensors
        if dimage is None and dweights is None:
            return None, None, None
        if dimage is None:
            dimage = torch.zeros((feat.shape[0], feat.shape[2] + 1), dtype=torch.float32, device=feat.device)
        dd, df = ops.ea_march_backward(dens, feat, ops._f32c(dimage), None if dweights is None else ops._f32c(dweights),
                                       ctx.threshold, need=ctx.needs_input_grad[:2])
        return dd, df, None


class EmissionAbsorptionRaymarcherStratified:
    """pren.py:256-369: rays_densities (..., P, 1) and rays_features (..., P, F) -> (images (..., F+1) [features |
    opacity], weights (..., P)) by ea_march above, which carries gradients to both inputs when they require one.
    thresholdMode marches the densities above `threshold` as ones.  The attributes stay assignable after construction
    (genFeat.py:132); weightMode and a surface_thickness other than 1 raise NotImplementedError when the marcher is called."""

    def __init__(self, surface_thickness: int = 1, thresholdMode: bool = False, weightMode: bool = False, threshold: float = 0.03):
        self.surface_thickness = surface_thickness
        self.thresholdMode = thresholdMode
        self.weightMode = weightMode
        self.threshold = threshold

    def march_threshold(self) -> float:
        """The threshold argument of the C entries: the marcher's own in thresholdMode, -1 (emission-absorption) otherwise."""
        if self.surface_thickness != 1:
            raise NotImplementedError("EmissionAbsorptionRaymarcherStratified: only surface_thickness = 1 is supported")
        if self.weightMode and not self.thresholdMode:
            raise NotImplementedError("EmissionAbsorptionRaymarcherStratified: weightMode is not supported")
        if not self.thresholdMode:
            return -1.0
        if not float(self.threshold) >= 0.0:
            raise ValueError(f"EmissionAbsorptionRaymarcherStratified: threshold = {self.threshold} must be >= 0 in thresholdMode")
        return float(self.threshold)

    def __call__(self, rays_densities: torch.Tensor, rays_features: torch.Tensor, **kwargs):
        thr = self.march_threshold()
        if rays_densities.shape[-1] != 1 or rays_features.shape[:-1] != rays_densities.shape[:-1]:
            raise ValueError(f"EmissionAbsorptionRaymarcherStratified: densities {tuple(rays_densities.shape)}, features "
                             f"{tuple(rays_features.shape)}: expected (..., P, 1) and (..., P, F)")
        return ea_march(rays_densities, rays_features, thr)

    forward = __call__


class ImplicitRendererStratified:
    """pren.py:57-253: renderer(cameras, volumetric_function, stratified=False, maskRays=False, mask=False) ->
    (images (..., F+1), ray_bundle, weights (..., P)).  The bundle is raysampler(cameras), (B, H, W, .) for a grid sampler,
    or with maskRays the (1, M, .) rays on non-zero pixels of `mask` (pren.py:230-236).  rayFreeze keeps the first call's
    bundle for every later call.  When volumetric_function is the bound batched_forward (or forward) of a
    fields.RadianceField the fused render runs; anything else callable is called as
    volumetric_function(ray_bundle=..., cameras=..., **kwargs) and its (densities, features) go through the raymarcher.

    stratified=True is the fine pass of pren.py:203-226 and needs a renderer built with fine_seed (an int): with the default
    fine_seed=None it raises NotImplementedError.  The coarse bundle is the one above; the reference selects the mask's rays
    after the coarse pass, this renderer before it — weights are per ray, so the rays and their weights are the same, for
    less work.  The coarse weights are emission-absorption weights whatever the marcher's thresholdMode (getWeights,
    pren.py:159-170): from field.render(threshold=-1) for a fused RadianceField, otherwise from the callable's densities
    through ops.ea_march(threshold=-1).  The fine bundle is ProbabilisticRaysampler(P, True, False, add_input_samples,
    seed=fine_seed) of the coarse bundle and weights ((..., 2P) lengths with add_input_samples, (..., P) without); the field
    and the marcher then run on it as above, and rayFreeze freezes it.  coarse=(bundle, weights) skips the coarse pass
    (pren2.py:204-217 with trainNerfFine.py:293-300's coarseR / coarseW).  A caller who wants fresh samples per call changes
    renderer.fine_seed."""

    def __init__(self, raysampler, raymarcher, device=None, rayFreeze: bool = False, fine_seed: int | None = None):
        if not callable(raysampler):
            raise ValueError('"raysampler" has to be a "Callable" object.')
        if not callable(raymarcher):
            raise ValueError('"raymarcher" has to be a "Callable" object.')
        self.raysampler, self.raymarcher, self.device, self.rayFreeze = raysampler, raymarcher, device, rayFreeze
        self.fine_seed = fine_seed
        self.rayState = "Empty"
        self.frozenRays = False

    @staticmethod
    def _fused_field(volumetric_function):
        from .fields import RadianceField
        owner = getattr(volumetric_function, "__self__", None)
        if isinstance(owner, RadianceField) and getattr(volumetric_function, "__func__", None) in (
                RadianceField.batched_forward, RadianceField.forward):
            return owner
        return None

    def _coarse_weights(self, bundle: RayBundle, cameras, volumetric_function, kwargs) -> torch.Tensor:
        """getWeights (pren.py:159-170): the emission-absorption weights of the field along the coarse bundle."""
        field = self._fused_field(volumetric_function)
        if field is not None:
            return field.render(bundle, threshold=-1.0, return_weights=True)[1]
        rays_densities, rays_features = volumetric_function(ray_bundle=bundle, cameras=cameras, **kwargs)
        return ea_march(rays_densities, rays_features, -1.0)[1]

    def __call__(self, cameras, volumetric_function, stratified: bool = False, maskRays: bool = False, mask=False,
                 add_input_samples: bool = False, coarse=None, **kwargs):
        if not callable(volumetric_function):
            raise ValueError('"volumetric_function" has to be a "Callable" object.')
        if stratified and self.fine_seed is None:
            raise NotImplementedError("ImplicitRendererStratified: stratified=True (ProbabilisticRaysampler) is not supported "
                                      "without fine_seed: build the renderer with fine_seed=<int>")
        if self.rayState == "Empty":
            if self.rayFreeze:
                self.rayState = "Occupied"
            if stratified and coarse is not None:
                bundle, weights = coarse
            else:
                bundle = self.raysampler(cameras, mask=mask) if maskRays else self.raysampler(cameras)
            if stratified:
                if coarse is None:
                    weights = self._coarse_weights(bundle, cameras, volumetric_function, kwargs)
                psampler = ProbabilisticRaysampler(bundle.lengths.shape[-1], True, False, add_input_samples, seed=self.fine_seed)
                bundle = psampler(bundle, weights)
            self.frozenRays = bundle
        bundle = self.frozenRays
        field = self._fused_field(volumetric_function)
        if field is not None and isinstance(self.raymarcher, EmissionAbsorptionRaymarcherStratified):
            images, weights, _ = field.render(bundle, threshold=self.raymarcher.march_threshold(), return_weights=True)
        else:
            rays_densities, rays_features = volumetric_function(ray_bundle=bundle, cameras=cameras, **kwargs)
            images, weights = self.raymarcher(rays_densities=rays_densities, rays_features=rays_features, ray_bundle=bundle, **kwargs)
        return images, bundle, weights

    forward = __call__
