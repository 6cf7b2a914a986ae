#!/usr/bin/env python3
"""Generates ref_radiance_render.npz: the fixture that pins the radiance field and its render to the reference's EXECUTED code.

  HarmonicEmbedding nerf.py:106-144 and NeuralRadianceFieldFeat nerf.py:148-767 (siren=False, mode="color"; used of it:
      __init__ :149-218, _get_densities :220-228, _get_colors :230-268, forward :340-402)
  EmissionAbsorptionRaymarcherStratified pren.py:256-369 (__init__ :287-297, forward :298-369) at thresholdMode False and
      True with threshold 0.2
  get_emb_vis nutil.py:198-210 and normImage nutil.py:345-348

As make_ref_fields.py does (its helpers are reused, its stand-ins and their caveats hold here too): nothing of the reference is
imported or stored, the named classes and functions are parsed with `ast`, compiled and executed, and only DATA is written.

Nets.  `big` is the default (60, 256) net and `small` a (4, 32) net, built in make_ref_fields.make_density_net's order under
its seeds, so that the trunks ARE ref_density_net.npz's (asserted here; the test reads them from there, which keeps this file
under the size limit).  The density row is re-parameterised as there.  The big net's first colour matrix is rounded to
bfloat16 values and stored as their upper 16 bits: parameter DATA edited after construction, no reference code changed.

Rays.  125 (big, P = 64) and 250 (small, P = 16) rays from a sphere of radius 2.5 towards the cube, every ray with its own
unnormalised direction (norms 0.7 to 4.7).

The f64 values follow make_ref_fields.py's "same args" construction: the .double() module's mlp, _get_densities and
color_layer on the sines and cosines of the f32 module's own embedding arguments (points and normalised directions), widened.
E_ref is the largest deviation of the f32 results from them: of the per-point colours, and of the soft-mode images marched by
the same marcher in f64.  In threshold mode a ray whose f64 densities come within 4 E_ref of 0.2 may be excused; asserted
here: those are at most CAP of the rays, and on every other ray the f32 and the f64 march choose the same sample (the f64
march keeps the marcher's eps of 1e-10, which f32 rounds away: its weights differ from 0 and 1 by about 1e-10).

Run from the repo root:  python tests/golden/make_ref_render.py
"""
import copy
import sys
from pathlib import Path
from typing import Callable, Tuple, Union

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_from_reference import OUT, ref_function                                                # noqa: E402
from make_ref_back_march import _shifted_cumprod                                                         # noqa: E402
from make_ref_fields import CAP, RayBundle, _embed_args, _save, net_arrays, ray_bundle_to_ray_points, ref_class, reparam_half   # noqa: E402

f32, f64 = np.float32, np.float64
THRESHOLD = 0.2


def ref_classes():
    ns = {"torch": torch, "np": np, "RayBundle": RayBundle, "ray_bundle_to_ray_points": ray_bundle_to_ray_points, "Siren": None,
          "Callable": Callable, "Tuple": Tuple, "Union": Union, "_shifted_cumprod": _shifted_cumprod,
          "_check_raymarcher_inputs": lambda *a, **k: None, "_check_density_bounds": lambda *a, **k: None}
    ref_class("nerf.py", "HarmonicEmbedding", 106, {"__init__": (107, 133), "forward": (135, 144)},
              ("x[..., None] * self.frequencies", "torch.cat((embed.sin(), embed.cos()), dim=-1)"), ns)
    NRF = ref_class("nerf.py", "NeuralRadianceFieldFeat", 148,
                    {"__init__": (149, 218), "_get_densities": (220, 228), "_get_colors": (230, 268), "forward": (340, 402)},
                    ("torch.nn.functional.normalize(rays_directions, dim=-1)", "torch.cat((features, rays_embedding_expand), dim=-1)",
                     "torch.nn.Linear(n_hidden_neurons + embedding_dim, n_hidden_neurons)", "torch.nn.Sigmoid()",
                     "self._get_colors(features, ray_bundle.directions)", "1 - (-raw_densities).exp()"), ns)
    EA = ref_class("pren.py", "EmissionAbsorptionRaymarcherStratified", 256, {"__init__": (287, 297), "forward": (298, 369)},
                   ("c1[torch.where(rays_densities > self.threshold)] = 1", "weights = rays_densities * absorption",
                    "features = (weights[..., None] * rays_features).sum(dim=-2)",
                    "opacities = 1.0 - torch.prod(1.0 - rays_densities, dim=-1, keepdim=True)",
                    "torch.cat((features, opacities), dim=-1), weights"), ns)
    return NRF, EA


def bundle(rng, R, P):
    o = rng.normal(size=(R, 3))
    o = 2.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
    t = rng.uniform(-0.6, 0.6, (R, 3))
    s = rng.uniform(0.4, 1.6, (R, 1))
    d = ((t - o) * s).astype(f32)
    ln = (np.linspace(0.2, 1.8, P)[None, :] / s + rng.uniform(0, 0.01, (R, P))).astype(f32)
    return RayBundle(torch.from_numpy(o.astype(f32))[None], torch.from_numpy(d)[None], torch.from_numpy(np.sort(ln, axis=1))[None], None)


@torch.no_grad()
def same_args64(model, m64, rb):
    """The .double() module's layers on the f32 module's own embedding arguments, of the points and of the directions."""
    def emb(x):
        e = _embed_args(model, x).double()
        return torch.cat((e.sin(), e.cos()), dim=-1)
    feats = m64.mlp(emb(ray_bundle_to_ray_points(rb)))
    dn = torch.nn.functional.normalize(rb.directions, dim=-1)
    e_dir = emb(dn)[..., None, :].expand(*feats.shape[:-1], 6 * len(model.harmonic_embedding.frequencies))
    return m64._get_densities(feats), m64.color_layer(torch.cat((feats, e_dir), dim=-1))


def main():
    NRF, EA = ref_classes()
    rng0 = np.random.default_rng(20261101)               # make_ref_fields.make_density_net's construction, step for step
    torch.manual_seed(20261101)
    big, small = NRF(), NRF(n_harmonic_functions=4, n_hidden_neurons=32)
    rng0.uniform(-1.2, 1.2, (2049, 3))
    stored = np.load(OUT / "ref_density_net.npz")
    out = {}
    rng = np.random.default_rng(20261201)
    for model, tag, R, P in ((big, "big", 125, 64), (small, "small", 250, 16)):
        assert not model.siren and model.mode == "color"
        reparam_half(model, rng0)
        for k, v in net_arrays(model, tag).items():
            assert np.array_equal(v, stored[k]), f"{k}: the trunk is not ref_density_net.npz's"
        c0, c2 = model.color_layer[0], model.color_layer[2]
        with torch.no_grad():
            c0.weight.data = c0.weight.data.bfloat16().float()
        w16 = (c0.weight.detach().numpy().view(np.uint32) >> 16).astype(np.uint16)
        assert np.array_equal((w16.astype(np.uint32) << 16).view(f32), c0.weight.detach().numpy())
        g = lambda t: t.detach().numpy().copy()
        out.update({f"{tag}_Wc1_bf16": w16, f"{tag}_bc1": g(c0.bias), f"{tag}_Wc2": g(c2.weight), f"{tag}_bc2": g(c2.bias)})
        rb = bundle(rng, R, P)
        m64 = copy.deepcopy(model).double()
        with torch.no_grad():
            dens, col = model.forward(rb)
            assert dens.shape == (1, R, P, 1) and col.shape == (1, R, P, 3) and col.dtype == torch.float32
            d64, c64 = same_args64(model, m64, rb)
        share = float((dens > THRESHOLD).float().mean())
        assert 0.15 <= share <= 0.85, f"{tag}: {share:.2f} of the samples above {THRESHOLD}"
        e_dens = float((dens.double() - d64).abs().max())
        e_col = float((col.double() - c64).abs().max())
        out.update({f"{tag}_origins": g(rb.origins), f"{tag}_directions": g(rb.directions), f"{tag}_lengths": g(rb.lengths),
                    f"{tag}_directions_normed": g(torch.nn.functional.normalize(rb.directions, dim=-1)),
                    f"{tag}_dens32": g(dens), f"{tag}_col32": g(col), f"{tag}_dens64": g(d64), f"{tag}_col64": g(c64),
                    f"{tag}_E_ref_dens": f64(e_dens), f"{tag}_E_ref_col": f64(e_col)})
        for mode, name in ((False, "soft"), (True, "thr")):
            marcher = EA(thresholdMode=mode, threshold=THRESHOLD)
            with torch.no_grad():
                img, w = marcher.forward(dens.clone(), col.clone())
                img64, w64 = marcher.forward(d64.clone(), c64.clone())
            assert img.shape == (1, R, 4) and w.shape == (1, R, P) and img64.dtype == torch.float64
            out.update({f"{tag}_{name}_image32": g(img), f"{tag}_{name}_weights32": g(w), f"{tag}_{name}_image64": g(img64)})
            if not mode:
                out[f"{tag}_E_ref_image"] = f64(float((img.double() - img64).abs().max()))
            else:
                near = ((d64[..., 0] - THRESHOLD).abs() <= 4 * e_dens).any(dim=-1)[0]
                assert float(near.float().mean()) <= CAP, f"{tag}: {int(near.sum())} of {R} rays near the threshold"
                # in f64 the marcher's eps does not vanish: the weights are (1 + 1e-10)^k at the first hit and about 1e-10
                # behind it.  The same sample is chosen where the largest f64 weight sits on the f32 weight's one.
                assert torch.equal((w64[0] > 0.5)[~near], (w[0] == 1)[~near])
                hit = (w != 0).any(dim=-1)[0]
                assert 0.3 <= float(hit.float().mean()) and (img[0, :, 3] == hit.float()).all()
                print(f"{tag}: {int(near.sum())} of {R} rays near the threshold, {float(hit.float().mean()):.2f} hit")
        print(f"{tag}: share above {THRESHOLD} {share:.2f}, E_ref dens {e_dens:.3e} col {e_col:.3e} image {out[f'{tag}_E_ref_image']:.3e}")
        assert 0 < e_col < 1e-4 and 0 < out[f"{tag}_E_ref_image"] < 1e-4 and float(col.std()) > 0.01
    # nutil's two image helpers on a rendered feature image
    ns = {"torch": torch}
    get_emb_vis, norm_image = ref_function("nutil.py", "get_emb_vis", ns), ref_function("nutil.py", "normImage", ns)
    emb = torch.from_numpy(rng.standard_normal((6, 7, 12)).astype(f32))
    mask = torch.from_numpy(rng.uniform(size=(6, 7)) > 0.3)
    out.update({"vis_emb": g(emb), "vis_mask": mask.numpy().astype(np.uint8),
                "vis_plain": g(get_emb_vis(emb.clone())), "vis_masked_demeaned": g(get_emb_vis(emb.clone(), mask, True)),
                "vis_norm_image": g(norm_image(emb.clone()))})
    _save("ref_radiance_render.npz", out)
    assert (OUT / "ref_radiance_render.npz").stat().st_size <= 1 << 20


if __name__ == "__main__":
    main()
