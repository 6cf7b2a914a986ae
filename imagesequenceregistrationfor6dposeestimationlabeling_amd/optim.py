"""The optimiser of the two training programs: torch.optim.Adam as trainPose.py:208-236, :450 and trainNerfFine.py:214, :354
use it, as one launch per step over every tensor of every group (include/isr_adam.h; isr_adam_step), with the arithmetic owned
by the package: the parameters after a step are a function of (parameters, gradients, moments, step counts, group constants)
alone, bit-equal to the library's host build.

Adam is a torch.optim.Optimizer, so training.pose_train_step and training.nerf_train_step take it as they are.  What differs
from torch.optim.Adam:
  * trainPose.py:229-236's learning-rate ramp is `ramp_steps`: lr_t = lr * min(1, (t + 1) / ramp_steps), computed on the device
    from the tensor's own step counter.  The group's "lr" stays what the caller set, nothing is rewritten per iteration, and a
    captured step replays with the ramp.
  * the step counters live on the device and step() never reads them; state[p]["step"] is a 0-d int64 view of that array.
    state_dict() writes torch.optim.Adam's layout (step as a float32 host tensor, exp_avg, exp_avg_sq), and a state written
    by torch.optim.Adam loads.
  * zero_in_step=True stores +0 to every gradient in the step's own launch; the zero_grad() that follows does nothing and
    keeps the gradient tensors, so with the second step the table of pointers is stable and step() is two kernel launches.
Out of scope: amsgrad, maximize, decoupled weight decay, mixed precision, sparse gradients."""
from __future__ import annotations

import numpy as np

import torch

from . import ops

__all__ = ["Adam", "nerf_optimizer", "pose_optimizer"]

LR_MLP = 3e-5           # trainPose.py:76
LR_CNN = 3e-4           # trainPose.py:75
RAMP_STEPS = 2000       # trainPose.py:230
LR_NERF = 1e-3          # trainNerfFine.py:214


class Adam(torch.optim.Optimizer):
    """Adam over contiguous float32 device parameters, at most 8 groups.  Per group: lr, betas, eps, weight_decay (L2, added
    to the gradient) and ramp_steps (0: none)."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 ramp_steps: float = 0, zero_in_step: bool = False):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, ramp_steps=ramp_steps)
        super().__init__(params, defaults)
        self.zero_in_step = bool(zero_in_step)
        self._index()
        self._groups_host()                                                           # a ValueError now, not at the first step

    # ---- the parameters, in the order of state_dict()'s ids
    def _index(self) -> None:
        if len(self.param_groups) > ops.ADAM_MAX_GROUPS:
            raise ValueError(f"optim.Adam: {len(self.param_groups)} parameter groups, at most {ops.ADAM_MAX_GROUPS}")
        self._flat = [(p, gi) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        if not self._flat:
            raise ValueError("optim.Adam: no parameters")
        dev = self._flat[0][0].device
        for slot, (p, _) in enumerate(self._flat):
            if not p.is_cuda or p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                raise ValueError(f"optim.Adam: parameter {slot} ({tuple(p.shape)}, {p.dtype}, {p.device}) is not a contiguous "
                                 f"float32 tensor on {dev}")
        self._device = dev
        self._steps = torch.zeros(len(self._flat), dtype=torch.int64, device=dev)
        self._key = None                # (slot, address of p, address of p.grad) of every row of the uploaded table
        self._table = None              # (table bytes, chunk_start, T, chunks) on the device
        self._pinned = None
        self._zeroed = None             # [(gradient tensor, its version)] right after a zero_in_step step

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        if hasattr(self, "_flat"):                                                    # after construction: new slots, old counts
            old = {id(p): self._steps[s] for s, (p, _) in enumerate(self._flat)}
            self._index()
            for s, (p, _) in enumerate(self._flat):
                if id(p) in old:
                    self._steps[s] = old[id(p)]
                    if p in self.state:
                        self.state[p]["step"] = self._steps[s]

    def _groups_host(self) -> np.ndarray:
        rows = []
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay"):
                raise ValueError("optim.Adam: amsgrad, maximize and decoupled weight decay are not supported")
            b1, b2 = g["betas"]
            row = [float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), float(g["ramp_steps"])]
            if not (row[0] >= 0 and 0 <= row[1] < 1 and 0 <= row[2] < 1 and row[3] > 0 and row[4] >= 0 and row[5] >= 0) \
                    or not np.isfinite(row).all():
                raise ValueError(f"optim.Adam: lr, betas, eps, weight_decay, ramp_steps = {row} "
                                 "(lr, weight_decay, ramp_steps >= 0, 0 <= beta < 1, eps > 0)")
            rows.append(row)
        return np.asarray(rows, np.float64)

    # ---- the table
    def _current_key(self) -> list:
        key = []
        for slot, (p, _) in enumerate(self._flat):
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or g.is_sparse or not g.is_contiguous():
                raise ValueError(f"optim.Adam: the gradient of parameter {slot} must be contiguous float32 of the parameter's shape")
            key.append((slot, p.data_ptr(), g.data_ptr()))
        return key

    def _ensure_table(self, key: list) -> None:
        """Rebuilds and uploads the table when a pointer in it has changed: one pinned buffer, one non-blocking copy."""
        if key == self._key and self._table is not None:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("optim.Adam: a gradient or parameter moved since the last step, so the table would have to be "
                               "uploaded inside a graph capture; capture with stable gradients (run one step first, and use "
                               "zero_in_step=True or zero_grad(set_to_none=False))")
        table = np.zeros(len(key), ops.ADAM_TENSOR)
        for i, (slot, p_ptr, g_ptr) in enumerate(key):
            p, gi = self._flat[slot]
            st = self.state[p]
            if len(st) == 0:
                st["step"] = self._steps[slot]
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            table[i] = (p_ptr, g_ptr, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), gi, slot)
        chunk_start, chunks = ops.adam_table_host(table, len(self.param_groups), len(self._flat))
        T = len(key)
        nbytes = T * ops.ADAM_TENSOR.itemsize
        pinned = torch.empty(nbytes + 4 * (T + 1), dtype=torch.uint8).pin_memory()
        host = pinned.numpy()
        host[:nbytes] = table.view(np.uint8)
        host[nbytes:] = chunk_start.view(np.uint8)
        with torch.cuda.device(self._device):
            dev = torch.empty(pinned.shape, dtype=torch.uint8, device=self._device)
            dev.copy_(pinned, non_blocking=True)
        self._pinned = pinned                                                         # alive until the next upload
        self._table = (dev[:nbytes], dev[nbytes:].view(torch.int32), T, chunks)
        self._key = key

    # ---- torch.optim.Optimizer
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        key = self._current_key()
        self._zeroed = None
        if not key:
            return loss
        self._ensure_table(key)
        table, chunk_start, T, chunks = self._table
        ops.adam_step(table, chunk_start, T, chunks, self._groups_host(), self._steps, zero_grads=self.zero_in_step)
        if self.zero_in_step:
            self._zeroed = [(p.grad, p.grad._version) for p, _ in self._flat if p.grad is not None]
        return loss

    def _still_zeroed(self) -> bool:
        if self._zeroed is None:
            return False
        grads = [p.grad for p, _ in self._flat if p.grad is not None]
        return len(grads) == len(self._zeroed) and all(g is z and g._version == ver for g, (z, ver) in zip(grads, self._zeroed))

    @torch.no_grad()
    def zero_grad(self, set_to_none: bool | None = None) -> None:
        """set_to_none=True: torch's meaning, every gradient becomes None.  False: +0 to every gradient in one launch, through
        the step's table.  None (the default): True, unless zero_in_step, where the gradients the last step zeroed are kept
        (nothing is launched when nothing touched them since)."""
        if set_to_none is None:
            set_to_none = not self.zero_in_step
        if set_to_none:
            for p, _ in self._flat:
                p.grad = None
            self._zeroed = None
            return
        if self._still_zeroed():
            return
        key = self._current_key()
        if not key:
            return
        for slot, _, _ in key:
            g = self._flat[slot][0].grad
            if g.grad_fn is not None:
                g.detach_()
            g.requires_grad_(False)
        self._ensure_table(key)
        table, chunk_start, T, chunks = self._table
        ops.adam_zero_grads(table, chunk_start, T, chunks)

    def state_dict(self) -> dict:
        """torch.optim.Adam's layout: per parameter step (a float32 host tensor), exp_avg, exp_avg_sq.  Reads the counters."""
        sd = super().state_dict()
        steps = self._steps.cpu().tolist()
        slot_of = {id(p): s for s, (p, _) in enumerate(self._flat)}
        ids = [i for g in sd["param_groups"] for i in g["params"]]
        flat = [p for g in self.param_groups for p in g["params"]]
        state = {}
        for i, p in zip(ids, flat):
            if i in sd["state"]:
                st = dict(sd["state"][i])
                st["step"] = torch.tensor(float(steps[slot_of[id(p)]]), dtype=torch.float32)
                state[i] = st
        return {"state": state, "param_groups": sd["param_groups"]}

    def load_state_dict(self, state_dict: dict) -> None:
        ramps = [g["ramp_steps"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, ramp in zip(self.param_groups, ramps):
            g.setdefault("ramp_steps", ramp)
        self._groups_host()
        steps = self._steps.cpu()
        for slot, (p, _) in enumerate(self._flat):
            st = self.state.get(p)
            if not st:
                steps[slot] = 0
                continue
            t = st["step"]
            steps[slot] = int(round(float(t.item() if isinstance(t, torch.Tensor) else t)))
            for k in ("exp_avg", "exp_avg_sq"):
                if st[k].shape != p.shape:
                    raise ValueError(f"optim.Adam: {k} of parameter {slot} has shape {tuple(st[k].shape)}, not {tuple(p.shape)}")
                # a copy of its own: torch hands over the saved tensors themselves when dtype and device already match
                st[k] = torch.zeros_like(p, memory_format=torch.contiguous_format).copy_(st[k])
        self._steps.copy_(steps)
        for slot, (p, _) in enumerate(self._flat):
            if self.state.get(p):
                self.state[p]["step"] = self._steps[slot]
        self._key = self._table = self._zeroed = None


def pose_optimizer(field, encoder, *, lr_mlp: float = LR_MLP, lr_cnn: float = LR_CNN, ramp_steps: float = RAMP_STEPS,
                   zero_in_step: bool = True) -> Adam:
    """trainPose.py:208-236's optimiser: the key field at lr_mlp, the encoder at lr_cnn, both ramped over the first
    ramp_steps iterations."""
    return Adam([{"params": list(field.parameters()), "lr": lr_mlp}, {"params": list(encoder.parameters()), "lr": lr_cnn}],
                ramp_steps=ramp_steps, zero_in_step=zero_in_step)


def nerf_optimizer(coarse, fine, *, lr: float = LR_NERF, zero_in_step: bool = True) -> Adam:
    """trainNerfFine.py:214's optimiser: the coarse and the fine field, one group each, no ramp."""
    return Adam([{"params": list(coarse.parameters()), "lr": lr}, {"params": list(fine.parameters()), "lr": lr}],
                zero_in_step=zero_in_step)
