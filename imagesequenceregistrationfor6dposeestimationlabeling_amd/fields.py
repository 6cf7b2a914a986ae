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


def _host_bundle(origins, directions, lengths):
    """-> contiguous f32 NumPy origins (N,3), directions (N,3), lengths (N,P) for a _host call, and N, P."""
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    ln = np.ascontiguousarray(lengths, np.float32)
    return o, d, ln, *ln.shape


def _width_chain(name: str, Ws, bs, first=None) -> tuple:
    """The widths of a chain of layers, checked: every W (out_l, in_l) with in_l the width before it (`first`, or W_0's own
    when None, at l = 0) and b (out_l,)."""
    widths = [(Ws[0].shape[1] if Ws[0].ndim == 2 else -1) if first is None else first]
    for l, (w, b) in enumerate(zip(Ws, bs)):
        if w.ndim != 2 or w.shape[1] != widths[-1] or b.shape[0] != w.shape[0]:
            raise ValueError(f"{name}: layer {l} has W {tuple(w.shape)} and b {tuple(b.shape)} after width {widths[-1]}")
        widths.append(w.shape[0])
    return tuple(int(v) for v in widths)


class _PackedField:
    """What the two fields share: layers to contiguous f32 on the host with their chain of widths checked, the pack made by
    the library and uploaded, and the checks in front of a device call.  `_host_calls` finishes the subclass's refusal."""

    @staticmethod
    def _host(t) -> np.ndarray:
        return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float32)

    def _layers(self, weights, biases, first=None):
        """-> (Ws, bs, widths): every W (out_l, in_l) with in_l the width before it, `first` (W_0's own when None) at l = 0."""
        Ws, bs = [self._host(w) for w in weights], [self._host(b).reshape(-1) for b in biases]
        return Ws, bs, _width_chain(type(self).__name__, Ws, bs, first)

    def _pack_and_upload(self, kind, dims, before, Ws, bs, after, device):
        """isr_<kind>_pack_bytes(*dims), isr_<kind>_pack(*dims, *before, W, b, *after, pack, bytes) -> (pack_host, pack): the
        pack and its copy on `device`, which is set.  device=None: host-only (the _host calls, the tests' reference), pack is
        None; there is no CPU fallback."""
        name, L = type(self).__name__, lib()
        nbytes = getattr(L, f"isr_{kind}_pack_bytes")(*dims)
        if nbytes == 0:
            raise IsrError(f"isr_{kind}_pack_bytes failed: {L.isr_last_error().decode()}")
        pack_host = np.empty(nbytes // 4, np.float32)
        check(getattr(L, f"isr_{kind}_pack")(*dims, *before, _vp(np.concatenate([w.reshape(-1) for w in Ws])),
                                             _vp(np.concatenate(bs)), *after, _vp(pack_host), nbytes), f"isr_{kind}_pack")
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise IsrError(f"{name}: device {self.device} is not a GPU (there is no CPU fallback)")
        return pack_host, None if self.device is None else torch.from_numpy(pack_host).to(self.device)

    def _need_device(self, *tensors):
        if self.pack is None:
            raise IsrError(f"{type(self).__name__} was built without a device (device=None): only {self._host_calls} available")
        require_cuda(self.pack, *tensors)

    def _rows(self, points: torch.Tensor) -> torch.Tensor:
        self._need_device(points)
        if points.shape[-1] != 3:
            raise ValueError(f"{type(self).__name__}: points {tuple(points.shape)} must end in 3")
        return points.to(torch.float32).reshape(-1, 3).contiguous()


class KeyField(_PackedField):
    """weights[l] (out_l, in_l), biases[l] (out_l,), omegas[l] a float (sine layer: h <- sin(omega (W h + b))) or None
    (linear layer: h <- W h + b); in_0 = 3, at most 8 layers, widths at most 256, the last at most 32."""
    _host_calls = "eval_host is"

    def __init__(self, weights, biases, omegas, device):
        if not (len(weights) == len(biases) == len(omegas)) or len(weights) == 0:
            raise ValueError(f"KeyField: {len(weights)} weights, {len(biases)} biases, {len(omegas)} omegas")
        Ws, bs, self.widths = self._layers(weights, biases)
        self.omegas = tuple(None if o is None else float(o) for o in omegas)
        self.n_layers = len(Ws)
        self.out_features = self.widths[-1]
        self._w = np.asarray(self.widths, np.int32)
        om = np.asarray([0.0 if o is None else o for o in self.omegas], np.float32)
        sine = np.asarray([o is not None for o in self.omegas], np.int32)
        self.pack_host, self.pack = self._pack_and_upload("field", (self.n_layers, _vp(self._w)), (), Ws, bs, (_vp(om), _vp(sine)),
                                                          device)

    @classmethod
    def from_linears(cls, linears, omegas, device=None):
        """From torch.nn.Linear modules (each with a bias), e.g. the linear of every SineLayer of the loaded feature_layer."""
        linears = list(linears)
        if any(m.bias is None for m in linears):
            raise ValueError("KeyField.from_linears: every layer needs a bias")
        if device is None:
            device = linears[0].weight.device
        return cls([m.weight for m in linears], [m.bias for m in linears], omegas, device)

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


class DensityField(_PackedField):
    """The density head of the reference's NeuralRadianceFieldFeat as a device-resident field: HarmonicEmbedding(H) ->
    Linear + Softplus(beta) per hidden layer -> Linear(., 1) + Softplus(beta) -> 1 - exp(-x) (nerf.py:106-144, :163-177,
    :206-228), evaluated by one kernel launch, and the ray march that turns it into surface points (pren.py:338-365 as
    genFeat.py:185-198 and generateCors.py:299-334 use it).  weights[l] (out_l, in_l) and biases[l] for the hidden layers
    (in_0 = 6 H, at most 4 layers of at most 256), then the output row (1, in) and its bias; frequencies (H,) f32, H <= 64."""

    _host_calls = "the _host calls are"

    def __init__(self, weights, biases, frequencies, beta=10.0, device=None):
        if len(weights) != len(biases) or len(weights) < 2:
            raise ValueError(f"DensityField: {len(weights)} weights, {len(biases)} biases (hidden layers, then the output row)")
        self.frequencies = self._host(frequencies).reshape(-1)
        self.H = int(self.frequencies.shape[0])
        Ws, bs, widths = self._layers(weights, biases, 6 * self.H)
        if widths[-1] != 1:
            raise ValueError(f"DensityField: the last layer has {widths[-1]} outputs, the density is one")
        self.widths = widths[1:-1]
        self.beta = float(beta)
        self._w = np.asarray(self.widths, np.int32)
        self.pack_host, self.pack = self._pack_and_upload("density", (len(self.widths), _vp(self._w), self.H),
                                                          (_vp(self.frequencies), self.beta), Ws, bs, (), device)

    @classmethod
    def from_linears(cls, hidden_linears, density_linear, n_harmonic=60, omega0=0.1, beta=10.0, device=None):
        """From the torch.nn.Linear modules of the loaded network: model.mlp[0], model.mlp[2] and model.density_layer[0].
        The frequencies are built as HarmonicEmbedding builds them (nerf.py:131-134)."""
        linears = list(hidden_linears) + [density_linear]
        if any(m.bias is None for m in linears):
            raise ValueError("DensityField.from_linears: every layer needs a bias")
        if device is None:
            device = linears[0].weight.device
        return cls([m.weight for m in linears], [m.bias for m in linears], cls.harmonic_frequencies(n_harmonic, omega0), beta,
                   device)

    @staticmethod
    def harmonic_frequencies(n_harmonic: int = 60, omega0: float = 0.1) -> torch.Tensor:
        """The `frequencies` buffer as HarmonicEmbedding builds it (nerf.py:131-134), (n_harmonic,) f32 on the host."""
        return (omega0 * (2.0 ** torch.arange(n_harmonic))).to(torch.float32)

    def customForwardForDensity(self, points: torch.Tensor) -> torch.Tensor:
        """nerf.py:417-432: points (..., 3) -> densities (..., 1), on the device."""
        return ops.density_eval(self.pack, self.widths, self.H, self._rows(points)).reshape(*points.shape[:-1], 1)

    def _bundle(self, origins, directions, lengths):
        self._need_device(origins, directions, lengths)
        if origins.shape[-1] != 3 or directions.shape != origins.shape or lengths.shape[:-1] != origins.shape[:-1]:
            raise ValueError(f"DensityField: origins {tuple(origins.shape)}, directions {tuple(directions.shape)}, lengths "
                             f"{tuple(lengths.shape)}: expected (..., 3), (..., 3), (..., P)")
        f = lambda t, c: t.to(torch.float32).reshape(-1, c).contiguous()
        return f(origins, 3), f(directions, 3), f(lengths, lengths.shape[-1])

    def batched_forward_fordensity(self, ray_bundle, n_batches: int = 16):
        """The reference's call of that name: any object with .origins, .directions (..., 3) and .lengths (..., P) ->
        (densities (..., P, 1), zeros (..., P, 3)).  The points origins + directions * lengths are made in the kernel;
        n_batches is accepted and changes nothing (rows are independent, the whole bundle is one launch)."""
        o, d, ln = self._bundle(ray_bundle.origins, ray_bundle.directions, ray_bundle.lengths)
        _, _, _, dens, _ = ops.density_march(self.pack, self.widths, self.H, o, d, ln, threshold=-1.0, want_densities=True)
        shape = tuple(ray_bundle.lengths.shape)
        return dens.reshape(*shape, 1), torch.zeros((*shape, 3), dtype=torch.float32, device=dens.device)

    def grid_densities(self, res: int = 128) -> torch.Tensor:
        """The (res, res, res) array batched_forward_forPC (nerf.py:676-700) hands to marching cubes, after its two
        movedims: out[i, j, k] = density(t[i], t[j], t[k]), t = linspace(-1, 1, res) in f64 rounded to f32."""
        self._need_device()
        t = torch.from_numpy(np.linspace(-1, 1, int(res)).astype(np.float32)).to(self.device)
        pts = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
        return ops.density_eval(self.pack, self.widths, self.H, pts).reshape(int(res), int(res), int(res))

    def batched_forward_forPC(self, threshold: float = 0.1, res: int = 128, coords: str = "reference"):
        """The reference's call of that name (nerf.py:640-703): grid_densities(res), then the iso-surface at `threshold` by
        ops.marching_cubes (the package's own rule, csrc/mc_extract.hpp; mcubes may triangulate ambiguous cells differently
        and orders its vertices differently) -> (mvertices (V,3) f64, mtriangles (F,3) int32), NumPy.  coords:
          "reference": (v - res/2) / (res/2), the reference's own map (v - 64) / 64 (nerf.py:701) for any res.  It is NOT the
                       grid's geometry: linspace(-1, 1, 128) has spacing 2/127, so index 127, the far face at +1, lands at
                       0.984 and every distance is scaled by 127/128.  It is what the reference saves and what its later
                       stages were tuned on;
          "grid":      -1 + 2 v / (res - 1), where the densities were evaluated;
          "index":     v, as marching cubes returns it."""
        if coords not in ("reference", "grid", "index"):
            raise ValueError(f"DensityField.batched_forward_forPC: coords = {coords!r} (reference, grid or index)")
        res = int(res)
        verts, tris = ops.marching_cubes(self.grid_densities(res), float(threshold))
        return self._pc_coords(verts.cpu().numpy(), res, coords), tris.cpu().numpy()

    @staticmethod
    def _pc_coords(v: np.ndarray, res: int, coords: str) -> np.ndarray:
        if coords == "reference":
            return (v - res / 2) / (res / 2)
        if coords == "grid":
            return -1.0 + 2.0 * v / (res - 1)
        return v

    def surface_points(self, origins, directions, lengths, threshold: float = 0.2, return_weights: bool = False,
                       surface_thickness: int = 1, direction: str = "front"):
        """genFeat.py:191-193: origins + directions * max(lengths * weights) per ray -> (points (..., 3), depth (...),
        hit (...) bool), and with return_weights the (..., P) weights of pren.py:365 as a fourth.  threshold >= 0 is the
        reference's thresholdMode (0.2 there); a negative one gives the emission-absorption weights.
        direction "back": the same triple for the march from the far end of the ray, the exit point (prenBack.py:378-381 as
        generateCors.py:334 reads it); "both": (front triple, back triple) from one launch, and with return_weights a third
        entry, the (..., 2P) weights [front | back] of prenBack.py:385."""
        if surface_thickness != 1:
            raise ValueError("DensityField.surface_points: only surface_thickness = 1 is supported")
        o, d, ln = self._bundle(origins, directions, lengths)
        pts, depth, hit, _, wts = ops.density_march(self.pack, self.widths, self.H, o, d, ln, threshold=threshold,
                                                    want_weights=return_weights, direction=direction)
        lead = tuple(lengths.shape[:-1])
        if direction == "both":
            res = tuple((pts[s].reshape(*lead, 3), depth[s].reshape(lead), hit[s].reshape(lead) != 0) for s in (0, 1))
            return res + (wts.reshape(*lead, -1),) if return_weights else res
        res = (pts.reshape(*lead, 3), depth.reshape(lead), hit.reshape(lead) != 0)
        return res + (wts.reshape(lengths.shape),) if return_weights else res

    def eval_host(self, points) -> np.ndarray:
        """The same field by the host build of the same header (isr_density_eval_host): NumPy (N,3) -> (N,).  For tests."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out = np.empty(pts.shape[0], np.float32)
        check(lib().isr_density_eval_host(_vp(self.pack_host), self.pack_host.nbytes, len(self.widths), _vp(self._w), self.H,
                                          _vp(pts), pts.shape[0], _vp(out)), "isr_density_eval_host")
        return out

    def grid_densities_host(self, res: int = 128) -> np.ndarray:
        """grid_densities by eval_host: NumPy (res, res, res) f32, the same points in the same order.  For tests."""
        t = np.linspace(-1, 1, int(res)).astype(np.float32)
        pts = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)
        return self.eval_host(pts).reshape(int(res), int(res), int(res))

    def march_host(self, origins, directions, lengths, threshold: float = 0.2, direction: str = "front"):
        """isr_density_march_host / isr_density_march_dir_host: NumPy (N,3), (N,3), (N,P) -> dict of points, depth, hit,
        densities, weights, shaped as ops.density_march shapes them for `direction`.  For tests."""
        o, d, ln, N, P = _host_bundle(origins, directions, lengths)
        way = ops.march_direction(direction)
        lead = (2, N) if way == 2 else (N,)
        out = dict(points=np.empty((*lead, 3), np.float32), depth=np.empty(lead, np.float32), hit=np.empty(lead, np.int32),
                   densities=np.empty((N, P), np.float32), weights=np.empty((N, 2 * P if way == 2 else P), np.float32))
        head = (_vp(self.pack_host), self.pack_host.nbytes, len(self.widths), _vp(self._w), self.H, _vp(o), _vp(d), _vp(ln), N, P,
                float(threshold))
        tail = (_vp(out["densities"]), _vp(out["weights"]), _vp(out["depth"]), _vp(out["points"]), _vp(out["hit"]))
        if way == 0:
            check(lib().isr_density_march_host(*head, *tail), "isr_density_march_host")
        else:
            check(lib().isr_density_march_dir_host(*head, way, *tail), "isr_density_march_dir_host")
        return out


class RadianceField(DensityField):
    """NeuralRadianceFieldFeat in mode="color" (nerf.py:163-218, :230-268, :340-402) as a device-resident field: the
    DensityField of the same trunk (every call of it keeps working, with the same bits) plus the colour head
    Linear(Wt + 6H -> Wc), Softplus(beta), Linear(Wc -> C), Sigmoid on the trunk's last activations and the harmonic
    embedding of the normalised ray direction, and the emission-absorption render of pren.py:298-369, fused into one call
    (include/isr_radiance.h states every rule).  weights / biases: the hidden layers, then the density row (1, Wt);
    color_weights / color_biases: W1 (Wc, Wt + 6H) with the trunk's columns first, W2 (C, Wc)."""

    def __init__(self, weights, biases, color_weights, color_biases, frequencies, beta=10.0, device=None):
        super().__init__(weights, biases, frequencies, beta, device)
        if len(color_weights) != 2 or len(color_biases) != 2:
            raise ValueError(f"RadianceField: {len(color_weights)} colour weights, {len(color_biases)} colour biases (two layers)")
        Wt = self.widths[-1]
        cW, cb, cw = self._layers(color_weights, color_biases, Wt + 6 * self.H)
        self.Wc, self.C = cw[1], cw[2]
        Ws, bs, _ = self._layers(weights, biases, 6 * self.H)
        self._source = (Ws, bs, cW, cb)      # host copies of the weights as given (TrainableRadianceField.from_radiance_field)
        self.rpack_host, self.rpack = self._pack_and_upload("radiance", (len(self.widths), _vp(self._w), self.H, self.Wc, self.C),
                                                            (_vp(self.frequencies), self.beta), Ws + cW, bs + cb, (), device)

    @classmethod
    def from_linears(cls, hidden_linears, density_linear, color_linears, n_harmonic=60, omega0=0.1, beta=10.0, device=None):
        """From the torch.nn.Linear modules of the loaded network: model.mlp[0], model.mlp[2], model.density_layer[0] and
        (model.color_layer[0], model.color_layer[2])."""
        trunk, colour = list(hidden_linears) + [density_linear], list(color_linears)
        if any(m.bias is None for m in trunk + colour):
            raise ValueError("RadianceField.from_linears: every layer needs a bias")
        if device is None:
            device = trunk[0].weight.device
        return cls([m.weight for m in trunk], [m.bias for m in trunk], [m.weight for m in colour], [m.bias for m in colour],
                   cls.harmonic_frequencies(n_harmonic, omega0), beta, device)

    @classmethod
    def from_module(cls, model, beta=10.0, device=None):
        """From a NeuralRadianceFieldFeat-shaped module: the Linear layers of .mlp, .density_layer and .color_layer and
        .harmonic_embedding.frequencies."""
        lin = lambda seq: [m for m in seq if isinstance(m, torch.nn.Linear)]
        trunk, colour = lin(model.mlp) + lin(model.density_layer), lin(model.color_layer)
        if device is None:
            device = trunk[0].weight.device
        return cls([m.weight for m in trunk], [m.bias for m in trunk], [m.weight for m in colour], [m.bias for m in colour],
                   model.harmonic_embedding.frequencies, beta, device)

    def _render(self, o, d, ln, **kw):
        return ops.radiance_render(self.rpack, self.widths, self.H, self.Wc, self.C, o, d, ln, **kw)

    def forward(self, ray_bundle, **kw):
        """nerf.py:340-402 in mode="color": any object with .origins, .directions (..., 3) and .lengths (..., P) ->
        (densities (..., P, 1), colours (..., P, C)), on the device."""
        o, d, ln = self._bundle(ray_bundle.origins, ray_bundle.directions, ray_bundle.lengths)
        out = self._render(o, d, ln, threshold=-1.0, want_densities=True, want_colours=True)
        shape = tuple(ray_bundle.lengths.shape)
        return out["densities"].reshape(*shape, 1), out["colours"].reshape(*shape, self.C)

    __call__ = forward

    def batched_forward(self, ray_bundle, n_batches: int = 16, **kw):
        """nerf.py:458-521: the same pair.  n_batches is accepted and changes nothing: rows are independent, the bundle is
        one call."""
        return self.forward(ray_bundle)

    def render(self, ray_bundle, threshold: float = -1.0, return_weights: bool = True):
        """The render of the bundle in one fused call: (images (..., C+1) [features | opacity], weights (..., P) or None,
        depth (...)).  threshold >= 0 is the raymarcher's thresholdMode."""
        o, d, ln = self._bundle(ray_bundle.origins, ray_bundle.directions, ray_bundle.lengths)
        out = self._render(o, d, ln, threshold=threshold, want_weights=return_weights)
        lead = tuple(ray_bundle.lengths.shape[:-1])
        wts = out["weights"].reshape(ray_bundle.lengths.shape) if return_weights else None
        return out["image"].reshape(*lead, self.C + 1), wts, out["depth"].reshape(lead)

    def render_host(self, origins, directions, lengths, threshold: float = -1.0):
        """isr_radiance_render_host: NumPy (N,3), (N,3), (N,P) -> dict of image, depth, points, hit, weights, densities,
        colours.  For tests."""
        o, d, ln, N, P = _host_bundle(origins, directions, lengths)
        out = dict(image=np.empty((N, self.C + 1), np.float32), depth=np.empty(N, np.float32), points=np.empty((N, 3), np.float32),
                   hit=np.empty(N, np.int32), weights=np.empty((N, P), np.float32), densities=np.empty((N, P), np.float32),
                   colours=np.empty((N, P, self.C), np.float32))
        check(lib().isr_radiance_render_host(_vp(self.rpack_host), self.rpack_host.nbytes, len(self.widths), _vp(self._w), self.H,
                                             self.Wc, self.C, _vp(o), _vp(d), _vp(ln), N, P, float(threshold),
                                             *(_vp(out[k]) for k in ("image", "depth", "points", "hit", "weights", "densities",
                                                                      "colours"))), "isr_radiance_render_host")
        return out


class FeatureField:
    """NeuralRadianceFieldFeat in mode="feature" with the SIREN head (nerf.py:388-390; genFeat.py:131, trainPose.py:165,
    generateCors.py:177 set it): the densities of a DensityField and the keys of a KeyField at the bundle's points
    origins + lengths * directions, which are materialised as the reference materialises them.  Hand its batched_forward to
    rays.ImplicitRendererStratified; the images come from ops.ea_march."""

    def __init__(self, density_field: DensityField, key_field: KeyField):
        self.density_field, self.key_field = density_field, key_field

    def forward(self, ray_bundle, **kw):
        pts = ray_bundle.origins[..., None, :] + ray_bundle.lengths[..., :, None] * ray_bundle.directions[..., None, :]
        dens, _ = self.density_field.batched_forward_fordensity(ray_bundle)
        return dens, self.key_field(pts)

    __call__ = forward

    def batched_forward(self, ray_bundle, n_batches: int = 16, **kw):
        return self.forward(ray_bundle)


class _KeyFieldFunction(torch.autograd.Function):
    """rows (N, 3) -> (N, ld) through a TrainableKeyField's packs: isr_field_eval forward, isr_field_backward backward.  Only
    the points are saved; the backward recomputes the forward.  params: every W, then every b."""

    @staticmethod
    def forward(ctx, field, rows, ld, *params):
        pack, packT = field._packs()
        out = (torch.empty if ld == field.out_features else torch.zeros)((rows.shape[0], ld), dtype=torch.float32, device=rows.device)
        ops.field_eval(pack, field.widths, rows, out=out)
        ctx.widths, ctx.packs = field.widths, (pack, packT)
        ctx.save_for_backward(rows)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        rows, = ctx.saved_tensors
        nl = len(ctx.widths) - 1
        need = ctx.needs_input_grad[3:]
        dW, db = ops.field_backward(*ctx.packs, ctx.widths, rows, dout.to(torch.float32).contiguous(),
                                    need=(any(need[:nl]), any(need[nl:])))
        shapes = list(zip(ctx.widths[1:], ctx.widths[:-1]))
        gW = torch.split(dW, [o * i for o, i in shapes]) if dW is not None else [None] * nl
        gb = torch.split(db, [o for o, _ in shapes]) if db is not None else [None] * nl
        grads = [g.view(o, i) if g is not None and n else None for g, (o, i), n in zip(gW, shapes, need[:nl])]
        grads += [g if g is not None and n else None for g, n in zip(gb, need[nl:])]
        return (None, None, None, *grads)


class TrainableKeyField(torch.nn.Module):
    """KeyField with parameters: the SIREN feature head trainPose.py trains (feature_layer.requires_grad_(True)), evaluated
    by KeyField's kernel with the same bits and differentiated by isr_field_backward with respect to its weights and
    biases.  weights[l] (out_l, in_l) and biases[l] (out_l,) are ParameterLists in the standard layout, so optimizers,
    per-layer learning rates and state_dict work as usual; omegas[l] is a float (sine layer) or None (linear layer).  The
    packs the kernels read are rebuilt on the device (isr_field_pack_device) whenever gradients are enabled or a parameter
    changed.  Points get no gradient: a point tensor that requires one is refused."""

    def __init__(self, weights, biases, omegas, device=None):
        super().__init__()
        if not (len(weights) == len(biases) == len(omegas)) or len(weights) == 0:
            raise ValueError(f"TrainableKeyField: {len(weights)} weights, {len(biases)} biases, {len(omegas)} omegas")
        f = lambda t: torch.as_tensor(t, dtype=torch.float32).detach().to(device).clone().contiguous()
        Ws, bs = [f(w) for w in weights], [f(b).reshape(-1) for b in biases]
        self.widths = _width_chain("TrainableKeyField", Ws, bs)
        if lib().isr_field_pack_bytes(len(Ws), _vp(np.asarray(self.widths, np.int32))) == 0:
            raise IsrError(f"TrainableKeyField: {lib().isr_last_error().decode()}")
        self.omegas = tuple(None if o is None else float(o) for o in omegas)
        self.n_layers, self.out_features = len(Ws), self.widths[-1]
        self.weights = torch.nn.ParameterList([torch.nn.Parameter(w) for w in Ws])
        self.biases = torch.nn.ParameterList([torch.nn.Parameter(b) for b in bs])
        self._packed, self._packed_at = None, None

    @classmethod
    def from_linears(cls, linears, omegas, device=None):
        """From torch.nn.Linear modules (each with a bias); their values are copied."""
        linears = list(linears)
        if any(m.bias is None for m in linears):
            raise ValueError("TrainableKeyField.from_linears: every layer needs a bias")
        return cls([m.weight for m in linears], [m.bias for m in linears], omegas, linears[0].weight.device if device is None else device)

    @classmethod
    def from_key_field(cls, key_field: KeyField, device=None):
        """From a KeyField's packed weights (read back out of its host pack)."""
        pack, Ws, bs, off = key_field.pack_host, [], [], 64
        for K, O in zip(key_field.widths[:-1], key_field.widths[1:]):
            OP, mfma = (O + 31) // 32 * 32, K >= 32
            ks = (K + 7) // 8 * 8 if mfma else (K + 3) // 4 * 4
            j, k = np.meshgrid(np.arange(O), np.arange(K), indexing="ij")
            lane = (k & 1) * 32 + (j & 31)
            idx = ((((j >> 5) * (ks >> 3) + (k >> 3)) * 64 + lane) * 4 + ((k & 7) >> 1)) if mfma else j * ks + k
            Ws.append(pack[off + idx])
            bs.append(pack[off + OP * ks: off + OP * ks + O].copy())
            off += OP * ks + OP
        return cls(Ws, bs, key_field.omegas, key_field.device if device is None else device)

    @classmethod
    def siren(cls, hidden=256, hidden_layers=2, out=12, first_omega=30.0, hidden_omega=30.0, outermost_linear=False, seed=None,
              device=None):
        """Siren(in_features=3, hidden_features=hidden, hidden_layers=hidden_layers, out_features=out) with the initialisation
        of Sitzmann et al. 2020, sec. 3.2: first layer U(-1/in, 1/in), the others U(-sqrt(6/in)/omega, sqrt(6/in)/omega),
        biases torch.nn.Linear's U(-1/sqrt(in), 1/sqrt(in)).  The reference's dep/siren.py is not part of it, so this follows
        the paper, not a pinned file."""
        gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
        widths = [3] + [int(hidden)] * (int(hidden_layers) + 1) + [int(out)]
        n = len(widths) - 1
        omegas = [float(first_omega)] + [float(hidden_omega)] * (n - 1)
        if outermost_linear:
            omegas[-1] = None
        Ws, bs = [], []
        for l, (i, o) in enumerate(zip(widths[:-1], widths[1:])):
            lim = 1.0 / i if l == 0 else (6.0 / i) ** 0.5 / float(hidden_omega)
            Ws.append((torch.rand((o, i), generator=gen) * 2 - 1) * lim)
            bs.append((torch.rand((o,), generator=gen) * 2 - 1) / i ** 0.5)
        return cls(Ws, bs, omegas, device)

    def to_key_field(self, device="parameters") -> KeyField:
        """A frozen KeyField from the current weights, on the parameters' device by default (host-only, as KeyField's
        device=None, while they are on the CPU)."""
        if device == "parameters":
            device = self.weights[0].device if self.weights[0].is_cuda else None
        return KeyField([w.detach() for w in self.weights], [b.detach() for b in self.biases], self.omegas, device)

    def _params(self):
        return [*self.weights, *self.biases]

    def _packs(self):
        """(pack, packT) of the current parameters, fresh buffers whenever they are rebuilt (a saved backward keeps its own)."""
        at = tuple((p.data_ptr(), p._version) for p in self._params())
        if self._packed is None or torch.is_grad_enabled() or at != self._packed_at:
            with torch.no_grad():
                W = torch.cat([w.reshape(-1) for w in self.weights])
                b = torch.cat([v.reshape(-1) for v in self.biases])
                self._packed, self._packed_at = ops.field_pack_device(self.widths, W, b, self.omegas), at
        return self._packed

    def _eval(self, points: torch.Tensor, ld: int) -> torch.Tensor:
        if points.requires_grad:
            raise NotImplementedError("TrainableKeyField: points get no gradient (detach them)")
        require_cuda(points, *self._params())
        if points.shape[-1] != 3:
            raise ValueError(f"TrainableKeyField: points {tuple(points.shape)} must end in 3")
        rows = points.to(torch.float32).reshape(-1, 3).contiguous()
        return _KeyFieldFunction.apply(self, rows, ld, *self._params()).reshape(*points.shape[:-1], ld)

    def forward(self, points: torch.Tensor) -> torch.Tensor:
        """points (..., 3) -> keys (..., out), on the device, differentiable with respect to the parameters."""
        return self._eval(points, self.out_features)

    def batched_customForward(self, points: torch.Tensor, n_batches: int = 16) -> torch.Tensor:
        """nerf.py:404-457: (..., 3) -> (..., out + 1), the last channel zeros (nerf.py:415), which takes no gradient.
        n_batches is accepted and changes nothing: rows are independent, the whole input is one launch."""
        return self._eval(points, self.out_features + 1)


class _RadianceFieldFunction(torch.autograd.Function):
    """The bundle (N,3), (N,3), (N,P) -> (densities (N,P), colours (N,P,C)) through a TrainableRadianceField's packs:
    isr_radiance_render forward (threshold -1, densities and colours asked for), isr_radiance_backward backward.  Only the
    rays are saved; the backward recomputes the forward.  params: every W, then every b, in isr_radiance_pack's order."""

    @staticmethod
    def forward(ctx, field, o, d, ln, *params):
        pack, packT = field._packs()
        out = ops.radiance_render(pack, field.widths, field.H, field.Wc, field.C, o, d, ln, threshold=-1.0, want_densities=True,
                                  want_colours=True)
        ctx.shape, ctx.packs = (field.widths, field.H, field.Wc, field.C), (pack, packT)
        ctx.save_for_backward(o, d, ln)
        return out["densities"], out["colours"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_dens, d_col):
        o, d, ln = ctx.saved_tensors
        shapes = ops.radiance_param_shapes(*ctx.shape)
        nl = len(shapes)
        need = ctx.needs_input_grad[4:]
        f = lambda t: None if t is None else t.to(torch.float32).contiguous()
        dW, db = ops.radiance_backward(*ctx.packs, *ctx.shape, o, d, ln, f(d_dens), f(d_col),
                                       need=(any(need[:nl]), any(need[nl:])))
        gW = torch.split(dW, [a * b for a, b in shapes]) if dW is not None else [None] * nl
        gb = torch.split(db, [a for a, _ in shapes]) if db is not None else [None] * nl
        grads = [g.view(a, b) if g is not None and n else None for g, (a, b), n in zip(gW, shapes, need[:nl])]
        grads += [g if g is not None and n else None for g, n in zip(gb, need[nl:])]
        return (None, None, None, None, *grads)


class TrainableRadianceField(torch.nn.Module):
    """RadianceField with parameters: NeuralRadianceFieldFeat in mode="color" as trainNerfFine.py:174-186 trains it (mlp,
    density_layer and color_layer; feature_layer stays frozen and is not part of this field), evaluated by RadianceField's
    kernel with the same bits and differentiated by isr_radiance_backward with respect to its weights and biases.
    weights / biases: ParameterLists of the hidden layers, then the density row (1, Wt); color_weights / color_biases:
    W1 (Wc, Wt + 6H) with the trunk's columns first, W2 (C, Wc); `frequencies` (H,) is a buffer, as in the reference.  The packs
    the kernels read are rebuilt on the device (isr_radiance_pack_device) whenever gradients are enabled or a parameter
    changed.  The rays get no gradient: a bundle tensor that requires one is refused.  Not a RadianceField:
    rays.ImplicitRendererStratified sends it down its generic, differentiable route."""

    def __init__(self, weights, biases, color_weights, color_biases, frequencies, beta=10.0, device=None):
        super().__init__()
        if len(weights) != len(biases) or len(weights) < 2:
            raise ValueError(f"TrainableRadianceField: {len(weights)} weights, {len(biases)} biases (hidden layers, then the density row)")
        if len(color_weights) != 2 or len(color_biases) != 2:
            raise ValueError(f"TrainableRadianceField: {len(color_weights)} colour weights, {len(color_biases)} colour biases (two layers)")
        f = lambda t: torch.as_tensor(t, dtype=torch.float32).detach().to(device).clone().contiguous()
        fr = f(frequencies).reshape(-1)
        self.H = int(fr.shape[0])
        Ws, bs = [f(w) for w in weights], [f(b).reshape(-1) for b in biases]
        widths = _width_chain("TrainableRadianceField", Ws, bs, 6 * self.H)
        if widths[-1] != 1:
            raise ValueError(f"TrainableRadianceField: the last trunk layer has {widths[-1]} outputs, the density is one")
        self.widths = widths[1:-1]
        cW, cb = [f(w) for w in color_weights], [f(b).reshape(-1) for b in color_biases]
        cw = _width_chain("TrainableRadianceField", cW, cb, self.widths[-1] + 6 * self.H)
        self.Wc, self.C = cw[1], cw[2]
        self.beta = float(beta)
        if lib().isr_radiance_pack_bytes(len(self.widths), _vp(np.asarray(self.widths, np.int32)), self.H, self.Wc, self.C) == 0:
            raise IsrError(f"TrainableRadianceField: {lib().isr_last_error().decode()}")
        if not (self.beta > 0.0 and self.beta <= 3.0e38):
            raise ValueError(f"TrainableRadianceField: beta = {beta} must be positive and finite")
        self.weights = torch.nn.ParameterList([torch.nn.Parameter(w) for w in Ws])
        self.biases = torch.nn.ParameterList([torch.nn.Parameter(b) for b in bs])
        self.color_weights = torch.nn.ParameterList([torch.nn.Parameter(w) for w in cW])
        self.color_biases = torch.nn.ParameterList([torch.nn.Parameter(b) for b in cb])
        self.register_buffer("frequencies", fr)
        self._packed, self._packed_at = None, None

    @classmethod
    def from_linears(cls, hidden_linears, density_linear, color_linears, n_harmonic=60, omega0=0.1, beta=10.0, device=None):
        """From the torch.nn.Linear modules of the loaded network (RadianceField.from_linears' signature); values are copied."""
        trunk, colour = list(hidden_linears) + [density_linear], list(color_linears)
        if any(m.bias is None for m in trunk + colour):
            raise ValueError("TrainableRadianceField.from_linears: every layer needs a bias")
        if device is None:
            device = trunk[0].weight.device
        return cls([m.weight for m in trunk], [m.bias for m in trunk], [m.weight for m in colour], [m.bias for m in colour],
                   DensityField.harmonic_frequencies(n_harmonic, omega0), beta, device)

    @classmethod
    def from_module(cls, model, beta=10.0, device=None):
        """From a NeuralRadianceFieldFeat-shaped module (RadianceField.from_module's signature); values are copied."""
        lin = lambda seq: [m for m in seq if isinstance(m, torch.nn.Linear)]
        trunk, colour = lin(model.mlp) + lin(model.density_layer), lin(model.color_layer)
        if device is None:
            device = trunk[0].weight.device
        return cls([m.weight for m in trunk], [m.bias for m in trunk], [m.weight for m in colour], [m.bias for m in colour],
                   model.harmonic_embedding.frequencies, beta, device)

    @classmethod
    def from_radiance_field(cls, field: RadianceField, device=None):
        """From a RadianceField's weights (the copies its constructor kept on the host)."""
        return cls(*field._source, field.frequencies, field.beta, field.device if device is None else device)

    def to_radiance_field(self, device="parameters") -> RadianceField:
        """The frozen RadianceField of the current weights, on the parameters' device by default (host-only, as
        RadianceField's device=None, while they are on the CPU)."""
        if device == "parameters":
            device = self.weights[0].device if self.weights[0].is_cuda else None
        det = lambda ps: [p.detach() for p in ps]
        return RadianceField(det(self.weights), det(self.biases), det(self.color_weights), det(self.color_biases),
                             self.frequencies, self.beta, device)

    # NeuralRadianceFieldFeat's state_dict names (nerf.py:163-218): Sequential(Linear, Softplus, ...) numbers its Linears 0, 2, ...
    def _reference_names(self):
        names = [f"mlp.{2 * l}" for l in range(len(self.widths))] + ["density_layer.0", "color_layer.0", "color_layer.2"]
        return list(zip(names, [*self.weights, *self.color_weights], [*self.biases, *self.color_biases]))

    def reference_state_dict(self) -> dict:
        """The parameters under NeuralRadianceFieldFeat's key names (mlp.0.weight, ..., density_layer.0.*, color_layer.0.*,
        color_layer.2.*, harmonic_embedding.frequencies), detached copies: what trainNerfFine.py:228-235 stores as
        "model_state_dict"."""
        sd = {}
        for name, w, b in self._reference_names():
            sd[name + ".weight"], sd[name + ".bias"] = w.detach().clone(), b.detach().clone()
        sd["harmonic_embedding.frequencies"] = self.frequencies.detach().clone()
        return sd

    def load_reference_state_dict(self, sd) -> None:
        """Copy the values of a NeuralRadianceFieldFeat state_dict (or of a {"epoch", "model_state_dict"} checkpoint) into the
        parameters.  feature_layer.* keys are ignored; a missing key or another shape is an error."""
        if "model_state_dict" in sd:
            sd = sd["model_state_dict"]
        with torch.no_grad():
            for name, w, b in self._reference_names():
                for key, p in ((name + ".weight", w), (name + ".bias", b)):
                    if key not in sd:
                        raise KeyError(f"TrainableRadianceField.load_reference_state_dict: {key} is missing")
                    v = torch.as_tensor(sd[key])
                    if tuple(v.shape) != tuple(p.shape):
                        raise ValueError(f"TrainableRadianceField.load_reference_state_dict: {key} is {tuple(v.shape)}, "
                                         f"expected {tuple(p.shape)}")
                    p.copy_(v.to(p.device, torch.float32))
            key = "harmonic_embedding.frequencies"
            if key in sd:
                v = torch.as_tensor(sd[key]).reshape(-1)
                if v.shape[0] != self.H:
                    raise ValueError(f"TrainableRadianceField.load_reference_state_dict: {v.shape[0]} frequencies, H = {self.H}")
                self.frequencies.copy_(v.to(self.frequencies.device, torch.float32))
        self._packed = None

    def _params(self):
        return [*self.weights, *self.color_weights, *self.biases, *self.color_biases]

    def _packs(self):
        """(pack, packT) of the current parameters, fresh buffers whenever they are rebuilt (a saved backward keeps its own)."""
        at = tuple((p.data_ptr(), p._version) for p in [*self._params(), self.frequencies])
        if self._packed is None or torch.is_grad_enabled() or at != self._packed_at:
            with torch.no_grad():
                W = torch.cat([w.reshape(-1) for w in [*self.weights, *self.color_weights]])
                b = torch.cat([v.reshape(-1) for v in [*self.biases, *self.color_biases]])
                self._packed = ops.radiance_pack_device(self.widths, self.H, self.Wc, self.C, self.frequencies, self.beta, W, b)
                self._packed_at = at
        return self._packed

    def forward(self, ray_bundle, **kw):
        """nerf.py:340-402 in mode="color": any object with .origins, .directions (..., 3) and .lengths (..., P) ->
        (densities (..., P, 1), colours (..., P, C)), on the device, differentiable with respect to the parameters.  Keywords
        (the renderer's cameras=) are accepted and ignored."""
        o, d, ln = ray_bundle.origins, ray_bundle.directions, ray_bundle.lengths
        if o.requires_grad or d.requires_grad or ln.requires_grad:
            raise NotImplementedError("TrainableRadianceField: the rays get no gradient (detach the bundle)")
        require_cuda(o, d, ln, *self._params())
        if o.shape[-1] != 3 or d.shape != o.shape or ln.shape[:-1] != o.shape[:-1]:
            raise ValueError(f"TrainableRadianceField: origins {tuple(o.shape)}, directions {tuple(d.shape)}, lengths "
                             f"{tuple(ln.shape)}: expected (..., 3), (..., 3), (..., P)")
        f = lambda t, c: t.to(torch.float32).reshape(-1, c).contiguous()
        dens, col = _RadianceFieldFunction.apply(self, f(o, 3), f(d, 3), f(ln, ln.shape[-1]), *self._params())
        shape = tuple(ln.shape)
        return dens.reshape(*shape, 1), col.reshape(*shape, self.C)

    def batched_forward(self, ray_bundle, n_batches: int = 16, **kw):
        """nerf.py:458-521: the same pair.  n_batches is accepted and changes nothing: rows are independent, the bundle is
        one call."""
        return self.forward(ray_bundle, **kw)
