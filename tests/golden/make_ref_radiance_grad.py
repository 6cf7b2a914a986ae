#!/usr/bin/env python3
"""Generates ref_radiance_grad.npz: the fixture that pins the backward of the radiance field (include/isr_radiance_grad.h) to
the reference's EXECUTED code.

  HarmonicEmbedding nerf.py:106-144 and NeuralRadianceFieldFeat nerf.py:148-402 (__init__ :149-218, _get_densities :220-228,
      _get_colors :230-268, forward :340-402) with siren=False in mode="color", under torch autograd in f32 and in f64

As make_ref_fields.py does (its extraction is reused): nothing of the reference is imported or stored, the named classes are
parsed with `ast`, compiled and executed, and only DATA is written.

Two nets, (H = 60, hidden 32) and (H = 4, hidden 32), their density rows re-parametrised by make_ref_fields.reparam_half so
that the densities spread around 0.2 (the reference's initial bias of -1.5 gives 3e-8 everywhere), over 40 rays x 16
samples; and the H = 4 net once more as `hot`: the density row doubled and its bias raised until the median pre-activation
of the bundle's points is 2, so that about half of them sit in softplus's linear region (beta z > 20) and densities reach
0.99.
    loss = sum(densities * A) + sum(colours * B)        with fixed random A (40, 16, 1) and B (40, 16, 3)

The f64 side sees the f32 side's embedding ARGUMENTS (make_ref_fields.py's dens64_same_args): its harmonic embedding is
replaced by the sines and cosines, taken in f64, of the f32 products x * f of the f32 points and of the f32-normalised
directions; at H = 60 an f64 product would be another function.  Asserted: the replaced embedding on the f32 module gives the
f32 module's own bits.  The directions are drawn and kept where torch's f32 normalize, the f64 normalize rounded to f32 and
the library's rule (the f32 fmaf sum of squares, its root and the quotients each rounded once) agree bit for bit (asserted),
so that every implementation embeds the same unit vectors.

Stored per case: the inputs, the weights, every gradient array in f64 (g64_*), and per array E_*: the largest deviation of
the reference's own f32 gradient from the f64 one (asserted finite and non-zero).

Run from the repo root:  python tests/golden/make_ref_radiance_grad.py
"""
import copy
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_from_reference import OUT                                             # noqa: E402
from make_ref_fields import RayBundle, _save, ray_bundle_to_ray_points, ref_class, reparam_half   # noqa: E402
from tests.density_ref import fma32                                                    # noqa: E402
from typing import Callable, Tuple, Union                                              # noqa: E402

f32, f64 = np.float32, np.float64
PARAMS = ("mlp.0", "mlp.2", "density_layer.0", "color_layer.0", "color_layer.2")
N_RAYS, P = 40, 16


def ref_model_class():
    ns = {"torch": torch, "np": np, "RayBundle": RayBundle, "ray_bundle_to_ray_points": ray_bundle_to_ray_points, "Siren": None,
          "Callable": Callable, "Tuple": Tuple, "Union": Union}
    ref_class("nerf.py", "HarmonicEmbedding", 106, {"__init__": (107, 133), "forward": (135, 144)},
              ("register_buffer", "omega0 * 2.0 ** torch.arange(n_harmonic_functions)", "x[..., None] * self.frequencies",
               "torch.cat((embed.sin(), embed.cos()), dim=-1)"), ns)
    return ref_class("nerf.py", "NeuralRadianceFieldFeat", 148,
                     {"__init__": (149, 218), "_get_densities": (220, 228), "_get_colors": (230, 268), "forward": (340, 402)},
                     ("torch.nn.Softplus(beta=10.0)", "1 - (-raw_densities).exp()", "torch.nn.functional.normalize(rays_directions, dim=-1)",
                      "torch.cat((features, rays_embedding_expand), dim=-1)", "elif self.mode == 'color'",
                      "rays_colors = self._get_colors(features, ray_bundle.directions)", "torch.nn.Linear(n_hidden_neurons, 3)"), ns)


class SameArgsEmbedding(torch.nn.Module):
    """nerf.py:143-144 with the product x * f taken in f32 whatever follows: the sines and cosines in `dtype`."""

    def __init__(self, frequencies32, dtype):
        super().__init__()
        self.register_buffer("frequencies", frequencies32.clone().float())
        self.dtype = dtype

    def forward(self, x):
        assert x.dtype == torch.float32
        embed = (x[..., None] * self.frequencies).view(*x.shape[:-1], -1).to(self.dtype)
        return torch.cat((embed.sin(), embed.cos()), dim=-1)


def library_normalize(d):
    """csrc/field_radiance.hpp's normalize3 restated: s = fmaf(d2, d2, fmaf(d1, d1, d0 * d0)); n = sqrt(s) rounded to f32; d / n
    rounded to f32."""
    s = fma32(d[:, 2], d[:, 2], fma32(d[:, 1], d[:, 1], (d[:, 0] * d[:, 0]).astype(f32)))
    n = np.sqrt(s.astype(f64)).astype(f32)
    return (d.astype(f64) / np.maximum(n, f32(1e-12)).astype(f64)[:, None]).astype(f32)


def draw_bundle(rng):
    o = rng.uniform(-1.5, 1.5, (400, 3)).astype(f32)
    d = (rng.standard_normal((400, 3)) * rng.uniform(0.3, 3.0, (400, 1))).astype(f32)
    t32 = torch.nn.functional.normalize(torch.from_numpy(d), dim=-1).numpy()
    t64 = torch.nn.functional.normalize(torch.from_numpy(d).double(), dim=-1).numpy().astype(f32)
    keep = np.where((t32.view(np.uint32) == t64.view(np.uint32)).all(axis=1)
                    & (t32.view(np.uint32) == library_normalize(d).view(np.uint32)).all(axis=1))[0][:N_RAYS]
    assert len(keep) == N_RAYS, f"only {len(keep)} of 400 directions normalise alike"
    o, d = o[keep], d[keep]
    ln = np.sort(rng.uniform(0.0, 2.0, (N_RAYS, P)), axis=1).astype(f32)
    return o, d, ln, t32[keep]


def grads(model, bundle, A, B, dtype):
    for p in model.parameters():
        p.grad = None
    dens, col = model(bundle)
    assert dens.dtype == dtype and col.dtype == dtype and dens.shape == (1, N_RAYS, P, 1) and col.shape == (1, N_RAYS, P, 3)
    ((dens * torch.from_numpy(A).to(dtype)).sum() + (col * torch.from_numpy(B).to(dtype)).sum()).backward()
    sd = dict(model.named_parameters())
    return ({f"{n}.{k}": sd[f"{n}.{k}"].grad.double().numpy().copy() for n in PARAMS for k in ("weight", "bias")},
            dens.detach()[0, :, :, 0].numpy(), col.detach()[0].numpy())


def main():
    NRF = ref_model_class()
    rng = np.random.default_rng(20261020)
    torch.manual_seed(20261020)
    o, d, ln, unit = draw_bundle(rng)
    bundle = RayBundle(torch.from_numpy(o)[None], torch.from_numpy(d)[None], torch.from_numpy(ln)[None], None)
    A, B = rng.standard_normal((N_RAYS, P, 1)).astype(f32), rng.standard_normal((N_RAYS, P, 3)).astype(f32)
    out = {"origins": o, "directions": d, "lengths": ln, "unit_directions": unit, "A": A, "B": B}
    nets = {"h60": NRF(n_harmonic_functions=60, n_hidden_neurons=32), "h4": NRF(n_harmonic_functions=4, n_hidden_neurons=32)}
    for m in nets.values():
        assert not m.siren and m.mode == "color"
        reparam_half(m, rng)
    hot = copy.deepcopy(nets["h4"])
    with torch.no_grad():
        hot.density_layer[0].weight.mul_(2.0)
        z = hot.density_layer[0](hot.mlp(hot.harmonic_embedding(ray_bundle_to_ray_points(bundle))))
        hot.density_layer[0].bias.add_(2.0 - z.median())            # the median of beta z at 20: softplus's seam
    nets["hot"] = hot
    for tag, model in nets.items():
        g32, dens32, col32 = grads(model, bundle, A, B, torch.float32)
        # the replaced embedding changes no bit of the f32 module
        same32 = copy.deepcopy(model)
        same32.harmonic_embedding = SameArgsEmbedding(model.harmonic_embedding.frequencies, torch.float32)
        g32b, dens32b, col32b = grads(same32, bundle, A, B, torch.float32)
        assert np.array_equal(dens32, dens32b) and np.array_equal(col32, col32b) and all(np.array_equal(g32[k], g32b[k]) for k in g32)
        m64 = copy.deepcopy(model).double()
        m64.harmonic_embedding = SameArgsEmbedding(model.harmonic_embedding.frequencies, torch.float64)
        g64, dens64, col64 = grads(m64, bundle, A, B, torch.float64)
        assert float(np.abs(dens32 - dens64).max()) < 1e-4 and float(np.abs(col32 - col64).max()) < 1e-4      # the same function
        z = (model.density_layer[0](model.mlp(same32.harmonic_embedding(ray_bundle_to_ray_points(bundle)))) * 10.0).detach()
        share = float((z > 20.0).float().mean())
        print(f"{tag}: densities {dens64.min():.3g} .. {dens64.max():.4g}, share in softplus's linear region {share:.2f}")
        if tag == "hot":
            assert 0.2 < share < 0.8 and dens64.max() > 0.99
        for name in PARAMS:
            lin = dict(model.named_modules())[name]
            out[f"{tag}_{name}.weight"], out[f"{tag}_{name}.bias"] = lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()
        out[f"{tag}_frequencies"] = model.harmonic_embedding.frequencies.numpy().copy()
        for k in g64:
            E = float(np.abs(g32[k] - g64[k]).max())
            assert np.isfinite(E) and E > 0 and np.isfinite(g64[k]).all(), (tag, k, E)
            out[f"{tag}_g64_{k}"], out[f"{tag}_E_{k}"] = g64[k], f64(E)
            print(f"   {k:24s} |g| <= {np.abs(g64[k]).max():.3g}  E {E:.3e}")
    _save("ref_radiance_grad.npz", out)
    assert (OUT / "ref_radiance_grad.npz").stat().st_size <= 1 << 20


if __name__ == "__main__":
    main()
