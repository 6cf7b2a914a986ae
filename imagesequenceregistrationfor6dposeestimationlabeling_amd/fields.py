"""KeyField: the key field of refine_pose as a device-resident coordinate MLP, evaluated by one kernel launch.

The reference builds its field as NeuralRadianceFieldFeat(siren=Siren) (inference.py:101) and asks it for the key
descriptors of the visible surface with batched_customForward (pose_refine.py:52-53): 16 chunk forwards through the feature
head Siren(in_features=3, out_features=12, hidden_features=256, hidden_layers=2) (nerf.py:201-202, 404-457) and a zero
channel appended (nerf.py:415).  A KeyField holds that head's weights packed for isr_field_eval and answers the same calls;
hand it to refine_pose / refine_poses / sequence.estimate_and_refine wherever they take `neural_radiance_field`.
A point's key is a function of the point and the weights only, so chunking is a no-op and a block of images is one call.
The reference's dep/siren.py is not part of it: depth, the omegas and whether the last layer is linear are arguments."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import ops
from ._capi import IsrError, check, lib, require_cuda


def _vp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


class KeyField:
    """weights[l] (out_l, in_l), biases[l] (out_l,), omegas[l] a float (sine layer: h <- sin(omega (W h + b))) or None
    (linear layer: h <- W h + b); in_0 = 3, at most 8 layers, widths at most 256, the last at most 32."""

    def __init__(self, weights, biases, omegas, device):
        if not (len(weights) == len(biases) == len(omegas)) or len(weights) == 0:
            raise ValueError(f"KeyField: {len(weights)} weights, {len(biases)} biases, {len(omegas)} omegas")
        host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float32)
        Ws, bs = [host(w) for w in weights], [host(b).reshape(-1) for b in biases]
        widths = [Ws[0].shape[1] if Ws[0].ndim == 2 else -1]
        for l, (w, b) in enumerate(zip(Ws, bs)):
            if w.ndim != 2 or w.shape[1] != widths[-1] or b.shape[0] != w.shape[0]:
                raise ValueError(f"KeyField: layer {l} has W {w.shape} and b {b.shape} after width {widths[-1]}")
            widths.append(w.shape[0])
        self.widths = tuple(int(v) for v in widths)
        self.omegas = tuple(None if o is None else float(o) for o in omegas)
        self.n_layers = len(Ws)
        self.out_features = self.widths[-1]
        L = lib()
        self._w = np.asarray(self.widths, np.int32)
        nbytes = L.isr_field_pack_bytes(self.n_layers, _vp(self._w))
        if nbytes == 0:
            raise IsrError(f"isr_field_pack_bytes failed: {L.isr_last_error().decode()}")
        om = np.asarray([0.0 if o is None else o for o in self.omegas], np.float32)
        sine = np.asarray([o is not None for o in self.omegas], np.int32)
        self.pack_host = np.empty(nbytes // 4, np.float32)
        check(L.isr_field_pack(self.n_layers, _vp(self._w), _vp(np.concatenate([w.reshape(-1) for w in Ws])),
                               _vp(np.concatenate(bs)), _vp(om), _vp(sine), _vp(self.pack_host), nbytes), "isr_field_pack")
        # device=None: host-only (eval_host, the tests' reference); there is no CPU fallback for the calls below
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise IsrError(f"KeyField: device {self.device} is not a GPU (there is no CPU fallback)")
        self.pack = None if self.device is None else torch.from_numpy(self.pack_host).to(self.device)

    @classmethod
    def from_linears(cls, linears, omegas, device=None):
        """From torch.nn.Linear modules (each with a bias), e.g. the linear of every SineLayer of the loaded feature_layer."""
        linears = list(linears)
        if any(m.bias is None for m in linears):
            raise ValueError("KeyField.from_linears: every layer needs a bias")
        if device is None:
            device = linears[0].weight.device
        return cls([m.weight for m in linears], [m.bias for m in linears], omegas, device)

    def _rows(self, points: torch.Tensor) -> torch.Tensor:
        if self.pack is None:
            raise IsrError("KeyField was built without a device (device=None): only eval_host is available")
        require_cuda(self.pack, points)
        if points.shape[-1] != 3:
            raise ValueError(f"KeyField: points {tuple(points.shape)} must end in 3")
        return points.to(torch.float32).reshape(-1, 3).contiguous()

    def __call__(self, points: torch.Tensor) -> torch.Tensor:
        """points (..., 3) -> keys (..., out), on the device."""
        return ops.field_eval(self.pack, self.widths, self._rows(points)).reshape(*points.shape[:-1], self.out_features)

    def batched_customForward(self, points: torch.Tensor, n_batches: int = 16) -> torch.Tensor:
        """nerf.py:404-457: (..., 3) -> (..., out + 1), the last channel zeros (nerf.py:415).  n_batches is accepted and
        changes nothing: rows are independent, the whole input is one launch."""
        rows = self._rows(points)
        out = torch.zeros((rows.shape[0], self.out_features + 1), dtype=torch.float32, device=rows.device)
        ops.field_eval(self.pack, self.widths, rows, out=out)
        return out.reshape(*points.shape[:-1], self.out_features + 1)

    def eval_host(self, points) -> np.ndarray:
        """The same field by the host build of the same header (isr_field_eval_host): NumPy (N,3) -> (N,out).  For tests."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out = np.empty((pts.shape[0], self.out_features), np.float32)
        check(lib().isr_field_eval_host(_vp(self.pack_host), self.pack_host.nbytes, self.n_layers, _vp(self._w), _vp(pts),
                                        pts.shape[0], _vp(out), self.out_features), "isr_field_eval_host")
        return out
