"""The contrastive key loss of trainPose.py on the device, with its gradient: nutil.returnCrossEntropyWithNeg
(trainPose.py:417, :423) and its siblings returnCrossEntropy and returnCrossEntropy2 (nutil.py:349-403) over the fused
kernels of include/isr_contrastive.h.  The (B, 1 + M, S) logits, their softmax and the gradient of both are never stored:
forward and backward recompute them tile by tile, so every negative of a key set is affordable, not a sample of them.

`contrastive_loss` is the torch.autograd.Function underneath; the three wrappers carry the reference's names and arguments.
Device tensors only: a CPU tensor raises IsrError, there is no CPU fallback.  Second derivatives are not provided.

`huber` is trainNerfFine.py's smooth L1 term (nutil.py:157-164): elementwise torch ops, on any device.

The ray losses of include/isr_ray_losses.h, device tensors only as well: `distortion_loss` / `mip360loss` is nutil.mip360loss
(nutil.py:140-152) without its (N, P-1, P-1) pair tensors, differentiable in the weights; `render_loss` is the Huber terms of
trainNerfFine.py:314-326 for one render, the targets read at the rays inside the kernel, differentiable in the render."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import ops

__all__ = ["contrastive_loss", "distortion_loss", "huber", "mip360loss", "render_loss", "returnCrossEntropy", "returnCrossEntropy2",
           "returnCrossEntropyWithNeg"]


class _ContrastiveLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, n, scale):
        q, k, n = (ops._f32c(x.detach()) for x in (q, k, n))
        m, t, _pos, _rows, loss = ops.contrastive_forward(q, k, n, scale)
        ctx.save_for_backward(q, k, n, m, t)
        ctx.scale = float(scale)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        q, k, n, m, t = ctx.saved_tensors
        g = grad.to(torch.float32).contiguous()          # stays on the device: the kernels read it there
        dq, dk, dn = ops.contrastive_backward(q, k, n, m, t, g, ctx.scale, need=ctx.needs_input_grad[:3])
        return dq, dk, dn, None


def contrastive_loss(q: torch.Tensor, k: torch.Tensor, n: torch.Tensor, scale: float = 1e-3) -> torch.Tensor:
    """scale * mean over the B S queries of the cross-entropy of (q_i . k_i, q_i . n_0, .., q_i . n_{M-1}) with target 0.
    q (B, S, D), k (B, S, D) the positive key of each query, n (B, M, D) or (1, M, D) (negatives shared by every batch item);
    D <= 64.  Differentiable in q, k and n (once); inputs that are not f32 or not contiguous are converted first, and the
    gradients come back in f32."""
    return _ContrastiveLoss.apply(q, k, n, scale)


def returnCrossEntropyWithNeg(q1, k1, k2, negFrac=1, device=False):
    """nutil.returnCrossEntropyWithNeg (nutil.py:368-385): q1, k1 (B, S, D), k2 (B, M, D) -> F.cross_entropy / 1000 (the kernels apply 1 / 1000 in f64 and round the loss once).  The
    reference's unused randperm is drawn as it draws it, so torch's host generator ends where the reference leaves it.
    Extension: k2 of shape (1, M, D) is one set of negatives shared by every batch item (it is not copied B times).
    `device` is accepted and ignored: the tensors say where they are."""
    torch.randperm(k1.shape[1], dtype=torch.int64)[0: int(k1.shape[1] * negFrac)]
    return contrastive_loss(q1, k1, k2, 1 / 1000)


def returnCrossEntropy(q1, k1, negFrac=1, device=False):
    """nutil.returnCrossEntropy (nutil.py:349-366): the negatives are int(S negFrac) of the batch's own keys, drawn by
    torch.randperm on the host generator as the reference draws them (the same seed gives the same negatives).  The gather
    k1[:, negKeys] stays a torch op, so its gradient is torch's."""
    negKeys = torch.randperm(k1.shape[1], dtype=torch.int64)[0: int(k1.shape[1] * negFrac)]
    return contrastive_loss(q1, k1, k1[:, negKeys, :], 1 / 1000)


def returnCrossEntropy2(q1, k1, negFrac=1, negKeys=1, device=False):
    """nutil.returnCrossEntropy2 (nutil.py:386-403): as returnCrossEntropy with the caller's negKeys (an index tensor)."""
    return contrastive_loss(q1, k1, k1[:, negKeys, :], 1 / 1000)


class _DistortionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lengths, weights):
        shape = weights.shape
        lengths, weights = (ops._f32c(x.detach()).reshape(-1, shape[-1]) for x in (lengths, weights))
        _, loss = ops.distortion_forward(lengths, weights, want_ray_loss=False)
        ctx.save_for_backward(lengths, weights)
        ctx.shape = shape
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        lengths, weights = ctx.saved_tensors
        g = grad.to(torch.float32).contiguous()          # stays on the device: the kernel reads it there
        return None, ops.distortion_backward(lengths, weights, g).reshape(ctx.shape)


def distortion_loss(lengths: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """The mean over the rays of sum_ij w_i w_j |ut_i - ut_j| + sum_i w_i^2 (t_{i+1} - t_i) / 3 over weights[..., :-1], t the
    depths scaled to [0, 1] and ut their midpoints (nutil.mip360loss).  lengths (..., P), weights (..., P), 2 <= P <= 1024.
    Differentiable in weights (once); lengths get no gradient, and a lengths that requires one raises NotImplementedError.
    Inputs that are not f32 or not contiguous are converted first, and the gradient comes back in f32."""
    if tuple(lengths.shape) != tuple(weights.shape) or weights.ndim < 1:
        raise ValueError(f"distortion_loss: lengths and weights must share a shape (..., P), got {tuple(lengths.shape)} and "
                         f"{tuple(weights.shape)}")
    if lengths.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("distortion_loss: no gradient for lengths (detach them)")
    return _DistortionLoss.apply(lengths, weights)


def mip360loss(ray_bundle, weights: torch.Tensor) -> torch.Tensor:
    """nutil.mip360loss (nutil.py:140-152): the distortion loss of a renderer's weights over its bundle's lengths."""
    return distortion_loss(ray_bundle.lengths, weights)


class _RenderLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendered, target_images, target_silhouettes, xys, scaling):
        B = xys.shape[0]
        args = (ops._f32c(rendered.detach()).reshape(B, -1, rendered.shape[-1]), ops._f32c(target_images.detach()),
                ops._f32c(target_silhouettes.detach()), ops._f32c(xys.detach()).reshape(B, -1, 2))
        ctx.save_for_backward(*args)
        ctx.scaling, ctx.shape = float(scaling), rendered.shape
        return ops.render_loss_forward(*args, scaling)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        g = grad.to(torch.float32).contiguous()          # both upstream values stay on the device
        return ops.render_loss_backward(*ctx.saved_tensors, g, ctx.scaling).reshape(ctx.shape), None, None, None, None


def render_loss(rendered: torch.Tensor, target_images: torch.Tensor, target_silhouettes: torch.Tensor, xys: torch.Tensor,
                scaling: float = 0.1):
    """trainNerfFine.py:314-326 for one render: rendered (B, ..., F+1) [colours | opacity], target_images (B, H, W, F),
    target_silhouettes (B, H, W), xys (B, ..., 2) -> (color_err, sil_err), the means of huber(render, target at the rays).abs()
    over the colours and over the opacity.  Differentiable in rendered (once); the targets and xys get no gradient."""
    out = _RenderLoss.apply(rendered, target_images, target_silhouettes, xys, scaling)
    return out[0], out[1]


def huber(x: torch.Tensor, y: torch.Tensor, scaling: float = 0.1) -> torch.Tensor:
    """nutil.huber (nutil.py:157-164): (sqrt(max(1 + (x - y)^2 / scaling^2, 1e-4)) - 1) * scaling, elementwise.  Torch's own
    kernels, forward and backward."""
    diff_sq = (x - y) ** 2
    return ((1 + diff_sq / (scaling ** 2)).clamp(1e-4).sqrt() - 1) * float(scaling)
