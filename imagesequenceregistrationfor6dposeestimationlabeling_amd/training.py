"""One optimisation step of trainPose.py through the package: the maskRays=True branch of trainPose.py:246-450, with the
queries sampled by rays.sample_images_at_mc_locs (whose backward is isr_sample_nearest_backward), the keys made by a
fields.TrainableKeyField (isr_field_backward) and the loss by losses.returnCrossEntropyWithNeg (isr_contrastive_backward): the
encoder and the key field are trained together, and every gradient the package computes is a function of its inputs only.

The encoder is unpinned: the reference's UNet (dep/unet.py) is not part of it, so `encoder` is any torch.nn.Module that maps
(B, 3, H, W) to (B, 13, H, W), and its own layers, forward and backward, are torch's.  Out of scope: the data loader, the
learning-rate ramp of trainPose.py:229-236, checkpoints, the back-face keys (computed by trainPose.py:380, unused by its
loss) and the maskRays=False branch."""
from __future__ import annotations

import torch

from . import losses, rays

__all__ = ["pose_train_step"]


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
