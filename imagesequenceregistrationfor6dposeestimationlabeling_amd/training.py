"""One optimisation step of trainPose.py through the package: the maskRays=True branch of trainPose.py:246-450, with the
queries sampled by rays.sample_images_at_mc_locs (whose backward is isr_sample_nearest_backward), the keys made by a
fields.TrainableKeyField (isr_field_backward) and the loss by losses.returnCrossEntropyWithNeg (isr_contrastive_backward): the
encoder and the key field are trained together, and every gradient the package computes is a function of its inputs only.

The encoder is unpinned: the reference's UNet (dep/unet.py) is not part of it, so `encoder` is any torch.nn.Module that maps
(B, 3, H, W) to (B, 13, H, W), and its own layers, forward and backward, are torch's.  Its arguments come from
augment.PoseBatches, the loader of dataGen.AugmentedSamples on the device (the warps, the paste and the ray remap of
augment.py; include/isr_augment.h), with the loader's colour augmentations under PoseBatches(color=True)
(include/isr_color_aug.h: owned definitions of the albumentations pass).  Out of scope: checkpoints, the
back-face keys (computed by trainPose.py:380, unused by its loss) and the maskRays=False branch.

nerf_train_step is one optimisation step of trainNerfFine.py:238-354 the same way: a coarse and a fine render through
rays.ImplicitRendererStratified, whose march carries gradients to the fields' densities and features (isr_ea_march_backward),
the targets sampled at the rays, and losses.huber — or, opt-in, losses.render_loss for the four Huber terms and
losses.mip360loss (nutil.py:140-152) as a distortion regulariser on both renders' weights (include/isr_ray_losses.h).  The two fields are unpinned: any callables that map a ray bundle to
(densities, features), differentiated by torch.  Out of scope: the loader, checkpoints, visualisation and trainNerfFine.py's
batch_idx bookkeeping (the caller passes the batch's cameras and targets)."""
from __future__ import annotations

import torch

from . import losses, rays

__all__ = ["nerf_train_step", "pose_train_step"]


def pose_train_step(encoder: torch.nn.Module, field, optimizer: torch.optim.Optimizer, rgb: torch.Tensor, mask: torch.Tensor,
                    pos_points: torch.Tensor, xys: torch.Tensor, neg_points: torch.Tensor, *, key_noise: float = 1e-3,
                    mask_weight: float = 1e-3, generator: torch.Generator | None = None) -> dict:
    """rgb (B, H, W, 3), mask (B, H, W) in [0, 1], pos_points (B, S, 3) the surface points of the rays at the NDC locations
    xys (B, S, 2), neg_points (1, B S, 3) (trainPose.py's negVec after its randperm), all on the device ->
    dict(loss, feature_loss, mask_loss) of detached 0-d tensors, after one optimizer step.  `field`: a
    fields.TrainableKeyField with 12 output channels.  `generator` draws the noise on the negatives (the device's default
    generator when None)."""
    B, S = int(xys.shape[0]), int(xys.shape[1])
    optimizer.zero_grad()                                                             # trainPose.py:246
    feat = torch.movedim(encoder(torch.movedim(rgb, 3, 1)), 1, 3)                     # :258
    if feat.ndim != 4 or feat.shape[-1] != 13:
        raise ValueError(f"pose_train_step: the encoder must give (B, 13, H, W), got {tuple(torch.movedim(feat, 3, 1).shape)}")
    mask_feat, feat12 = feat[..., -1:], feat[..., 0:12]                               # :261-263
    noise = torch.randn(neg_points.shape, dtype=neg_points.dtype, device=neg_points.device, generator=generator)
    neg_vec = neg_points + noise * key_noise                                          # :358-359
    neg_keys = field.batched_customForward(neg_vec)[..., 0:12].reshape(-1, 12).unsqueeze(0)      # :362-376
    key = field.batched_customForward(pos_points)[:, :, 0:12]                         # :379, :394
    queries = rays.sample_images_at_mc_locs(feat12, xys)                              # :397-400
    feature_loss = losses.returnCrossEntropyWithNeg(queries, key, neg_keys.view(B, S, -1))      # :423
    mask_loss = torch.nn.functional.binary_cross_entropy(torch.sigmoid(mask_feat[..., 0]), mask) * mask_weight      # :430
    loss = feature_loss + mask_loss                                                   # :432
    loss.backward()                                                                   # :449
    optimizer.step()                                                                  # :450
    return {"loss": loss.detach(), "feature_loss": feature_loss.detach(), "mask_loss": mask_loss.detach()}


def nerf_train_step(coarse_field, fine_field, renderer_coarse, renderer_fine, optimizer: torch.optim.Optimizer, cameras,
                    target_images: torch.Tensor, target_silhouettes: torch.Tensor, *, distortion_weight: float = 0.0,
                    fused_losses: bool = False) -> dict:
    """cameras: the batch's B rays.PerspectiveCameras; target_images (B, H, W, F) and target_silhouettes (B, H, W) on the
    device -> dict(loss, color_err, sil_err) of detached 0-d tensors, after one optimizer step.  The fields are callables
    (ray_bundle=..., cameras=...) -> (densities (..., P, 1), features (..., P, F)); renderer_coarse and renderer_fine are
    rays.ImplicitRendererStratified over a Monte-Carlo sampler, renderer_fine built with fine_seed.

    Both options are off by default, and the step then runs the statements it always ran.  distortion_weight > 0 adds
    distortion_weight * (mip360loss of the coarse render + mip360loss of the fine render) to the loss (nutil.mip360loss, which
    trainPose.py imports) and returns the unweighted sum under "distortion".  fused_losses=True computes the four Huber terms by
    two losses.render_loss calls (include/isr_ray_losses.h) in place of two samplings and four elementwise chains."""
    optimizer.zero_grad()                                                             # trainNerfFine.py:238
    rendered, sampled_rays, weights = renderer_coarse(cameras=cameras, volumetric_function=coarse_field,
                                                      add_input_samples=False, stratified=False)      # :288-291
    rendered_fine, sampled_rays2, weights2 = renderer_fine(cameras=cameras, volumetric_function=fine_field, add_input_samples=True,
                                                    stratified=True, coarse=(sampled_rays, weights.detach()))      # :294-300
    xys = sampled_rays2.xys                                                           # :301
    last = rendered.shape[-1]
    if fused_losses:                                                                  # :314-329 in two calls
        color_err, sil_err = losses.render_loss(rendered, target_images, target_silhouettes, xys)
        color_fine, sil_fine = losses.render_loss(rendered_fine, target_images, target_silhouettes, xys)
        sil_err, color_err = sil_err + sil_fine, color_err + color_fine
    else:
        images, silhouettes = rendered.split([last - 1, 1], dim=-1)                   # :306-308
        images_fine, silhouettes_fine = rendered_fine.split([last - 1, 1], dim=-1)    # :310-312
        silhouettes_at_rays = rays.sample_images_at_mc_locs(target_silhouettes[..., None], xys)      # :314-317
        colors_at_rays = rays.sample_images_at_mc_locs(target_images, xys)            # :320-323
        sil_err = losses.huber(silhouettes, silhouettes_at_rays).abs().mean()         # :324
        color_err = losses.huber(images, colors_at_rays).abs().mean()                 # :326
        sil_err = sil_err + losses.huber(silhouettes_fine, silhouettes_at_rays).abs().mean()      # :328
        color_err = color_err + losses.huber(images_fine, colors_at_rays).abs().mean()      # :329
    sil_err, color_err = 500 * sil_err, 500 * color_err                               # :334-335
    loss = color_err + sil_err                                                        # :336
    out = {}
    if distortion_weight > 0:
        distortion = losses.mip360loss(sampled_rays, weights) + losses.mip360loss(sampled_rays2, weights2)
        loss = loss + distortion_weight * distortion
        out["distortion"] = distortion.detach()
    loss.backward()                                                                   # :353
    optimizer.step()                                                                  # :354
    return {"loss": loss.detach(), "color_err": color_err.detach(), "sil_err": sil_err.detach(), **out}
