#!/usr/bin/env python3
"""Generates ref_ray_losses.npz: the fixture that pins the ray losses to the reference's EXECUTED code.

  mip360loss                nutil.py:140-152
  huber                     nutil.py:157-164
  sample_images_at_mc_locs  nutil.py:167-196

As make_ref_losses.py does: nothing of the reference is imported or stored, each function is parsed with `ast`, compiled and
executed on the CPU under torch autograd, and only DATA is written.  Every case runs in f32 and, with the same inputs widened,
in f64.  Stored per case: the inputs (f32), the f64 loss and gradient (what the tests compare with), the f32 loss, and for the
loss and the gradient the largest deviation of the f32 run from the f64 run (`*_eref`: what the tests' tolerance is measured
from; NaN entries, which both runs share, are left out of it).

Distortion cases, weights from an emission-absorption march of random densities (tests/ray_losses_ref.march_weights):
  small (37, 5) sorted random depths;  coarse (64, 64) linspace depths;  fine (48, 128) the fine pass's depths (half linspace,
  half random, sorted);  equal (9, 7) with row 4 all equal (its loss and gradient row are NaN).
Render case: B = 2, 9 x 9 targets, n = 40 with rays outside the image on each side and exact zeros of d, F = 3; the colour and
the opacity terms are trainNerfFine.py:314-326's: huber(render, sample_images_at_mc_locs(target, xys)).abs().mean(), and the
stored gradient is that of colour + 2 * opacity (so the two upstream values differ).

Run from the repo root:  python tests/golden/make_ref_ray_losses.py
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_from_reference import ref_function                                                      # noqa: E402
from make_ref_fields import _save                                                                        # noqa: E402
from tests import ray_losses_ref as ref                                                                  # noqa: E402

f32, f64 = np.float32, np.float64
SEED = 20261020


def deviation(a32, b64):
    """The largest |a - b| over the entries that are not NaN in both."""
    a, b = np.asarray(a32, f64), np.asarray(b64, f64)
    both = np.isnan(a) & np.isnan(b)
    assert (np.isnan(a) == np.isnan(b)).all()
    return np.array(np.abs(a - b)[~both].max() if (~both).any() else np.nan)


def run_distortion(fn, lengths, weights, dtype):
    w = torch.from_numpy(weights).to(dtype).requires_grad_(True)
    loss = fn(SimpleNamespace(lengths=torch.from_numpy(lengths).to(dtype)), w)
    loss.backward()
    return loss.detach().numpy(), w.grad.numpy()


def run_render(sample, huber, rendered, images, sils, xys, dtype):
    x = torch.from_numpy(rendered).to(dtype).requires_grad_(True)
    images, sils, xys = (torch.from_numpy(a).to(dtype) for a in (images, sils, xys))
    F = images.shape[-1]
    colours, opacity = x.split([F, 1], dim=-1)                                        # trainNerfFine.py:306-308
    sil_at = sample(sils[..., None], xys)                                             # :314-317
    col_at = sample(images, xys)                                                      # :320-323
    sil_err = huber(opacity, sil_at).abs().mean()                                     # :324
    col_err = huber(colours, col_at).abs().mean()                                     # :326
    (col_err + 2 * sil_err).backward()
    return np.stack([col_err.detach().numpy(), sil_err.detach().numpy()]), x.grad.numpy()


def main():
    ns = {"torch": torch}
    mip = ref_function("nutil.py", "mip360loss", ns)
    huber = ref_function("nutil.py", "huber", ns)
    sample = ref_function("nutil.py", "sample_images_at_mc_locs", ns)
    rng = np.random.default_rng(SEED)
    out = {"seed": np.array([SEED], np.int64)}
    cases = {
        "small": (np.sort(1 + 3 * rng.random((37, 5)), axis=1).astype(f32), ref.march_weights(rng, 37, 5)),
        "coarse": (np.broadcast_to(np.linspace(1.0, 4.0, 64, dtype=f32), (64, 64)).copy(), ref.march_weights(rng, 64, 64)),
        "fine": (ref.fine_depths(rng, 48, 128), ref.march_weights(rng, 48, 128)),
        "equal": (np.sort(1 + 3 * rng.random((9, 7)), axis=1).astype(f32), ref.march_weights(rng, 9, 7)),
    }
    cases["equal"][0][4] = 2.5
    for tag, (lengths, weights) in cases.items():
        l32, g32 = run_distortion(mip, lengths, weights, torch.float32)
        l64, g64 = run_distortion(mip, lengths, weights, torch.float64)
        assert l32.dtype == f32 and l64.dtype == f64
        out[f"{tag}_lengths"], out[f"{tag}_weights"] = lengths, weights
        out[f"{tag}_loss_f32"], out[f"{tag}_loss_f64"], out[f"{tag}_loss_eref"] = l32, l64, deviation(l32, l64)
        out[f"{tag}_dweights_f64"], out[f"{tag}_dweights_eref"] = g64, deviation(g32, g64)
        assert tag == "equal" or (np.isfinite(g64).all() and out[f"{tag}_dweights_eref"] > 0)
    assert np.isnan(out["equal_loss_f64"]) and np.isnan(out["equal_dweights_f64"][4, :-1]).all()
    assert np.isfinite(np.delete(out["equal_dweights_f64"], 4, axis=0)).all() and (out["equal_dweights_f64"][:, -1] == 0).all()

    rendered, images, sils, xys = ref.render_case(rng, 2, 40, 3, 9, 9)
    o32, g32 = run_render(sample, huber, rendered, images, sils, xys, torch.float32)
    o64, g64 = run_render(sample, huber, rendered, images, sils, xys, torch.float64)
    out["render_rendered"], out["render_images"], out["render_sils"], out["render_xys"] = rendered, images, sils, xys
    out["render_out_f32"], out["render_out_f64"] = o32, o64
    out["render_out_eref"] = np.abs(o32.astype(f64) - o64)
    out["render_upstream"] = np.array([1.0, 2.0], f32)
    out["render_drendered_f64"], out["render_drendered_eref"] = g64, deviation(g32, g64)
    assert (g64[:, 6:9] == 0).all() and out["render_drendered_eref"] > 0
    _save("ref_ray_losses.npz", out)


if __name__ == "__main__":
    main()
