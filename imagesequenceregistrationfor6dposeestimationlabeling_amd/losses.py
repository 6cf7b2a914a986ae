"""The contrastive key loss of trainPose.py on the device, with its gradient: nutil.returnCrossEntropyWithNeg
(trainPose.py:417, :423) and its siblings returnCrossEntropy and returnCrossEntropy2 (nutil.py:349-403) over the fused
kernels of include/isr_contrastive.h.  The (B, 1 + M, S) logits, their softmax and the gradient of both are never stored:
forward and backward recompute them tile by tile, so every negative of a key set is affordable, not a sample of them.

`contrastive_loss` is the torch.autograd.Function underneath; the three wrappers carry the reference's names and arguments.
Device tensors only: a CPU tensor raises IsrError, there is no CPU fallback.  Second derivatives are not provided.

`huber` is trainNerfFine.py's smooth L1 term (nutil.py:157-164): elementwise torch ops, on any device."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import ops

__all__ = ["contrastive_loss", "huber", "returnCrossEntropy", "returnCrossEntropy2", "returnCrossEntropyWithNeg"]


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


def huber(x: torch.Tensor, y: torch.Tensor, scaling: float = 0.1) -> torch.Tensor:
    """nutil.huber (nutil.py:157-164): (sqrt(max(1 + (x - y)^2 / scaling^2, 1e-4)) - 1) * scaling, elementwise.  Torch's own
    kernels, forward and backward."""
    diff_sq = (x - y) ** 2
    return ((1 + diff_sq / (scaling ** 2)).clamp(1e-4).sqrt() - 1) * float(scaling)
