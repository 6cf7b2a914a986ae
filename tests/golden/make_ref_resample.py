#!/usr/bin/env python3
"""Generates ref_resample.npz: the fixture that pins the fine pass's ray sampler to the reference's EXECUTED code.

  ProbabilisticRaysampler pren.py:372-457 (__init__ :383-405, forward :407-457)

As make_ref_fields.py and make_ref_render.py do (their helpers are reused): nothing of the reference is imported or stored,
the class is parsed with `ast`, compiled and executed, and only DATA is written.

What the class is given that is not the reference's.  `sample_pdf` is pytorch3d's, which is not available: the name is bound
to tests/resample_ref.sample_pdf_torch, the restatement of sample_pdf_python from memory, and where that would call
torch.rand it takes RECORDED units instead — the Philox units of include/isr_resample.h under SEED with the flattened ray
index as the ray id, so that the package's sampler can be asked for the same draw.  With det the units are
torch.linspace(0, 1, n), as in sample_pdf_python.  What the fixture pins is therefore forward's own code: the mid-points,
the [1:-1] slice of the weights, the det rule, the concatenation and the sort.  The rule of sample_pdf stays UNPINNED.

Cases.  Bundles of (2, 5, 8) and (1, 3, 3, 8) lengths, add_input_samples False and True, training True and False.  forward
views its samples as (batch, rays, n), so the 4-D bundle goes through the views of pren.py:216-224, restated in `run`.
Every case is run in f32 (what the test compares with) and, with the same units widened, in f64 (what its tolerance is
measured from).  The weights sum to about 0.4, so that no bin's cdf step comes near eps: asserted here, no sample of the
fixture falls under the excuse rule of tests/resample_ref.excused_f64.

Run from the repo root:  python tests/golden/make_ref_resample.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_ref_fields import RayBundle, _save, ref_class                                                  # noqa: E402
from tests import resample_ref as rf                                                                     # noqa: E402

f32, f64 = np.float32, np.float64
SEED = 11
SHAPES = {"b3": ((2, 5, 8), 8), "b4": ((1, 3, 3, 8), 6)}          # lengths' shape, n_pts_per_ray


class _Units:
    """The stand-in for sample_pdf: the restatement, fed the recorded units."""

    def __init__(self):
        self.det_seen = []

    def __call__(self, bins, weights, n, det=False, eps=1e-5):
        N = bins.shape[0]
        self.det_seen.append(bool(det))
        u = np.stack([rf.units(n, bool(det), SEED, i) for i in range(N)])
        self.u = u
        return rf.sample_pdf_torch(bins, weights, torch.from_numpy(u).to(bins.dtype), eps)


def ref_sampler(ns):
    return ref_class("pren.py", "ProbabilisticRaysampler", 372, {"__init__": (383, 405), "forward": (407, 457)},
                     ("0.5 * (z_vals[..., 1:] + z_vals[..., :-1])", "ray_weights.view(-1, ray_weights.shape[-1])[..., 1:-1]",
                      "det=not (self._stratified and self.training or (self._stratified_test and (not self.training)))",
                      "torch.cat((z_vals, z_samples), dim=-1)", "torch.sort(z_vals, dim=-1)"), ns)


def inputs(rng, shape):
    P = shape[-1]
    lead = int(np.prod(shape[:-1]))
    ln = np.sort(rng.uniform(0.5, 4.0, (lead, P)).astype(f32), axis=1)
    w = rng.uniform(0.0, 1.0, (lead, P)).astype(f32) ** 3
    w[rng.uniform(size=w.shape) < 0.3] = 0
    w = (w * f32(0.4) / w.sum(axis=1, keepdims=True)).astype(f32)
    return ln.reshape(shape), w.reshape(shape)


def run(cls, stand_in, ln, w, n, add, training, dtype):
    """forward on the bundle; a 4-D bundle through the views of pren.py:216-224."""
    ln_t, w_t = torch.from_numpy(ln).to(dtype), torch.from_numpy(w).to(dtype)
    o = torch.zeros((*ln.shape[:-1], 3), dtype=dtype)
    xy = torch.zeros((*ln.shape[:-1], 2), dtype=dtype)
    sampler = cls(n, stratified=True, stratified_test=False, add_input_samples=add)
    sampler.train(training)
    P = ln.shape[-1]
    if ln_t.ndim == 4:
        bsz = ln.shape[0]
        out = sampler(RayBundle(o.view(bsz, -1, 3), o.view(bsz, -1, 3), ln_t.view(bsz, -1, P), xy.view(bsz, -1, 2)), w_t)
        lengths = out.lengths.view(*ln.shape[:-1], -1)
    else:
        out = sampler(RayBundle(o, o, ln_t, xy), w_t)
        lengths = out.lengths
    return lengths.numpy()


def main():
    stand_in = _Units()
    cls = ref_sampler({"torch": torch, "RayBundle": RayBundle, "sample_pdf": stand_in})
    rng = np.random.default_rng(20240611)
    out = {"seed": np.array([SEED], np.int64)}
    for name, (shape, n) in SHAPES.items():
        ln, w = inputs(rng, shape)
        out[f"{name}_lengths"], out[f"{name}_weights"], out[f"{name}_n"] = ln, w, np.array([n], np.int64)
        for add in (False, True):
            for training in (True, False):
                tag = f"{name}_add{int(add)}_train{int(training)}"
                z32 = run(cls, stand_in, ln, w, n, add, training, torch.float32)
                assert stand_in.det_seen[-1] == (not training), "the det rule of pren.py:438-441"
                u = stand_in.u.copy()
                z64 = run(cls, stand_in, ln, w, n, add, training, torch.float64)
                assert z32.shape == (*shape[:-1], n + (shape[-1] if add else 0)) and z32.dtype == f32 and z64.dtype == f64
                assert not rf.excused_f64(w.reshape(-1, shape[-1])[:, 1:-1], u).any(), f"{tag}: a sample on the knife edge"
                out[f"{tag}_units"], out[f"{tag}_f32"], out[f"{tag}_f64"] = u, z32, z64
    _save("ref_resample.npz", out)


if __name__ == "__main__":
    main()
