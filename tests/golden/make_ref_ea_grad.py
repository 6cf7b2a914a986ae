#!/usr/bin/env python3
"""Generates ref_ea_grad.npz: the fixture that pins the backward of the emission-absorption march, and losses.huber, to the
reference's EXECUTED code.

  EmissionAbsorptionRaymarcherStratified pren.py:256-369 (__init__ :287-297, forward :298-369) at thresholdMode False, under
      torch autograd in f32 and in f64
  huber nutil.py:157-164

As make_ref_render.py does (its extraction and make_ref_back_march.py's _shifted_cumprod, supplied from memory of pytorch3d
and not pinned, are reused): nothing of the reference is imported or stored, the named class and function are parsed with
`ast`, compiled and executed, and only DATA is written.

Two shapes.  `train` is trainNerfFine.py's coarse pass (1 200 rays, P = 64, F = 3) cut to 40 rays; `wide` is (40, 256, 12).
Of the 40 rays 14 have uniform densities, 13 small ones (below 0.05) and 13 a sharp sigmoid across a surface; every density
is clipped to [0, 1 - 2^-10], so that the reference's own f32 gradient is finite (asserted): torch's cumprod backward divides
by 1 - c.  The features are sixty-fourths in [-2, 2), stored as int8.

The loss contracts the images with Wi (N, F + 1) and the weights with Ww (N, P), fixed random tensors, so that the gradient
with respect to the weights is exercised:  loss = sum(images * Wi) + sum(weights * Ww).
Stored: the inputs, the f64 gradient of the densities dd64, and E_dd, E_df: the largest deviation of the f32 gradients from
the f64 ones.  The f64 gradient of the features is stored as its two factors: autograd makes it as weights64[..., None] * Wi,
one f64 product, and that is asserted here bit for bit; the test multiplies them again.

Run from the repo root:  python tests/golden/make_ref_ea_grad.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_from_reference import OUT, ref_function                              # noqa: E402
from make_ref_back_march import _shifted_cumprod                                       # noqa: E402
from make_ref_fields import _save, ref_class                                           # noqa: E402

f32, f64 = np.float32, np.float64
TOP = 1.0 - 2.0 ** -10


def ref_marcher():
    ns = {"torch": torch, "_shifted_cumprod": _shifted_cumprod, "_check_raymarcher_inputs": lambda *a, **k: None,
          "_check_density_bounds": lambda *a, **k: None}
    return ref_class("pren.py", "EmissionAbsorptionRaymarcherStratified", 256, {"__init__": (287, 297), "forward": (298, 369)},
                     ("_shifted_cumprod(1.0 + eps - rays_densities, shift=self.surface_thickness)",
                      "weights = rays_densities * absorption", "features = (weights[..., None] * rays_features).sum(dim=-2)",
                      "opacities = 1.0 - torch.prod(1.0 - rays_densities, dim=-1, keepdim=True)",
                      "torch.cat((features, opacities), dim=-1), weights"), ns)


def densities(rng, N, P):
    n_uni, n_small = 14, 13
    x = np.linspace(-1, 1, P)[None, :] - rng.uniform(-0.5, 0.5, (N - n_uni - n_small, 1))
    rho = np.concatenate([rng.uniform(0, 1, (n_uni, P)), rng.uniform(0, 0.05, (n_small, P)), 1 / (1 + np.exp(-40 * x))])
    return np.clip(rho, 0.0, TOP).astype(f32)


def grads(marcher, rho, feat, Wi, Ww, dtype):
    d = torch.from_numpy(rho).to(dtype)[None, :, :, None].requires_grad_(True)
    f = torch.from_numpy(feat).to(dtype)[None].requires_grad_(True)
    images, weights = marcher.forward(d, f)
    assert images.dtype == dtype and images.shape == (1, *Wi.shape) and weights.shape == (1, *Ww.shape)
    ((images * torch.from_numpy(Wi).to(dtype)).sum() + (weights * torch.from_numpy(Ww).to(dtype)).sum()).backward()
    return d.grad[0, :, :, 0].numpy(), f.grad[0].numpy(), weights.detach()[0].numpy()


def main():
    marcher = ref_marcher()(thresholdMode=False)
    rng = np.random.default_rng(20261019)
    out = {}
    for tag, N, P, F in (("train", 40, 64, 3), ("wide", 40, 256, 12)):
        rho = densities(rng, N, P)
        q = rng.integers(-128, 128, (N, P, F)).astype(np.int8)
        feat = q.astype(f32) / f32(64)
        Wi, Ww = rng.standard_normal((N, F + 1)).astype(f32), rng.standard_normal((N, P)).astype(f32)
        dd32, df32, _ = grads(marcher, rho, feat, Wi, Ww, torch.float32)
        dd64, df64, w64 = grads(marcher, rho, feat, Wi, Ww, torch.float64)
        assert np.isfinite(dd32).all() and np.isfinite(df32).all() and rho.max() <= TOP and rho.min() >= 0
        assert np.array_equal(df64, w64[:, :, None] * Wi.astype(f64)[:, None, :-1]), "dfeatures is not weights x Wi, bit for bit"
        E_dd, E_df = float(np.abs(dd32 - dd64).max()), float(np.abs(df32 - df64).max())
        assert 0 < E_dd < 1e-3 * np.abs(dd64).max() and 0 < E_df < 1e-5 * np.abs(df64).max()
        print(f"{tag}: ({N}, {P}, {F})  |dd| <= {np.abs(dd64).max():.3g}, E_dd {E_dd:.3e};  |df| <= {np.abs(df64).max():.3g}, E_df {E_df:.3e}")
        out.update({f"{tag}_rho": rho, f"{tag}_feat_q": q, f"{tag}_Wi": Wi, f"{tag}_Ww": Ww, f"{tag}_dd64": dd64, f"{tag}_w64": w64,
                    f"{tag}_dd32": dd32, f"{tag}_E_dd": f64(E_dd), f"{tag}_E_df": f64(E_df)})
    # nutil.huber on rendered-like and target-like values, the default scaling and another
    huber = ref_function("nutil.py", "huber", {"torch": torch})
    x, y = rng.uniform(-0.2, 1.2, (40, 4)).astype(f32), rng.uniform(0, 1, (40, 4)).astype(f32)
    x[0], y[1, 0] = y[0], 30.0                           # exact zeros of the difference, and a large one
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    out.update({"huber_x": x, "huber_y": y, "huber_default32": huber(tx, ty).numpy(), "huber_default64": huber(tx.double(), ty.double()).numpy(),
                "huber_half32": huber(tx, ty, 0.5).numpy(), "huber_half64": huber(tx.double(), ty.double(), 0.5).numpy()})
    _save("ref_ea_grad.npz", out)
    assert (OUT / "ref_ea_grad.npz").stat().st_size <= 1 << 20


if __name__ == "__main__":
    main()
