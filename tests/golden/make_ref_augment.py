#!/usr/bin/env python3
"""Generates ref_augment.npz: the fixture that pins the ray remap and the candidate set of isr_augment_rays to the reference's
EXECUTED code.

  getNerfSamples augment.py:639-685 (the statements of lines 640-685; the NOCS map below them is out of scope)

As the other make_ref_*.py do: nothing of the reference is imported or stored, the statements are parsed with `ast`, compiled
and executed, and only DATA is written.

What the statements are given that is not the reference's.  `cv2` is not available: cv2.getRotationMatrix2D is bound to
augment.rotation_matrix_2d, the documented formula from memory (UNPINNED).  `torch.load` is bound to a lookup of in-memory
tensors by the path the statements build, so no file is read; every other name of `torch` is torch's.  The arguments are what
dataGen.AugmentedSamples passes (dataGen.py:84-85): trR = int(trR), trT and trS the f32 tensors generateImages returns.

What is recorded per case and set: the view's xys and positions, the f32 matrix and translation the package is to be given
(augment.ray_transform), the reference's remapped coordinates (s1, s2), its candidate set (idx_b2 / idx_b1, or every row when
the filter does not apply) and its sample `samps` — a randperm, compared only as a subset of the candidates.

Asserted here: no reference coordinate lies within the test's bound (tests/augment_ref.remap_bound) of +-1, except in case 1,
where rot 0 / scale 1 / t = 0 makes the arithmetic exact and rows sit at exactly 1.0 and nextafter(1, 0) on purpose.

Run from the repo root:  python tests/golden/make_ref_augment.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_from_reference import ref_statements                                                    # noqa: E402
from make_ref_fields import _save                                                                        # noqa: E402
from imagesequenceregistrationfor6dposeestimationlabeling_amd import augment                             # noqa: E402
from tests import augment_ref as ar                                                                      # noqa: E402

f32 = np.float32
IMD, SIZE = 224, 224
#        rot, scale, tra,        n front, n back, spread, S
CASES = ((37, 1.137, (10, -20), 300, 200, 0.9, 64),
         (0, 1.0, (0, 0), 40, 30, 0.95, 16),                 # exact arithmetic; rows at 1.0 and nextafter(1, 0) are added
         (90, 0.5, (3, 5), 120, 80, 0.9, 32),                # everything stays inside: the no-filter branch
         (271, 0.8, (-50, 40), 257, 129, 0.99, 300),         # S above the inside count
         (123, 0.9, (7, 11), 2100, 2049, 0.8, 512))


class _Cv2:
    getRotationMatrix2D = staticmethod(augment.rotation_matrix_2d)


class _Torch:
    """torch, with load() answering from memory."""

    def __init__(self, files):
        self._files = files

    def load(self, path):
        return self._files[path].clone()

    def __getattr__(self, name):
        return getattr(torch, name)


def main():
    code = ref_statements("augment.py", 640, 685,
                          ("cv2.getRotationMatrix2D((0, 0), trR, float(trS))", "torch.mm(s1, torch.from_numpy(M.astype('float32'))[0:2, 0:2].T) - trT / (imD / 2)",
                           "if s1.max() >= 1 or s1.min() <= -1:", "(s1[:, 0] > -1) & (s1[:, 0] < 1) & (s1[:, 1] > -1) & (s1[:, 1] < 1)",
                           "torch.randperm(idx_b2.shape[0], dtype=torch.int64)[0:sampleSize]"))
    rng = np.random.default_rng(20261020)
    torch.manual_seed(5)
    out = {"n_cases": np.array(len(CASES), np.int64), "imD": np.array(IMD, np.int64)}
    for c, (rot, scale, tra, n1, n2, spread, S) in enumerate(CASES):
        xy1, xy2 = (rng.uniform(-spread, spread, (n, 2)).astype(f32) for n in (n1, n2))
        if c == 1:
            xy1[3], xy1[7], xy2[5] = (1.0, 0.25), (np.nextafter(f32(1), f32(0)), -0.5), (-1.0, 0.0)
        p1, p2 = (rng.normal(size=(n, 3)).astype(f32) for n in (n1, n2))
        files = {f"nerf/{SIZE}_sampledRayxys/0.pt": torch.from_numpy(xy1)[None], f"nerf/{SIZE}_posVec/0.pt": torch.from_numpy(p1)[None],
                 f"nerf/{SIZE}_sampledRayBackxys/0.pt": torch.from_numpy(xy2)[None], f"nerf/{SIZE}_posVecBack/0.pt": torch.from_numpy(p2)[None]}
        trT, trS = torch.tensor(tra, dtype=torch.float32), torch.tensor([scale], dtype=torch.float32)      # augment.py:327-328, :357-358
        ns = {"torch": _Torch(files), "cv2": _Cv2, "np": np, "bid": 0, "nerfID": "nerf", "render_size": SIZE, "sampleSize": S, "imD": IMD,
              "trR": int(rot), "trT": trT, "trS": trS, "NOCS": False}
        exec(code, ns)
        rot4, t2 = augment.ray_transform([rot], [scale], [tra], IMD)
        out[f"c{c}_rot"], out[f"c{c}_t"], out[f"c{c}_S"] = rot4[0], t2[0], np.array(S, np.int64)
        for s, xy, pos, rem, idx_name, samp_pos, samp_xy in (("front", xy1, p1, ns["s1"], "idx_b2", ns["posVec1"], ns["sampled_raysxys1"]),
                                                            ("back", xy2, p2, ns["s2"], "idx_b1", ns["backVec1"], ns["backraysxys1"])):
            rem = rem.numpy()
            filtered = idx_name in ns
            cand = ns[idx_name].numpy() if filtered else np.arange(xy.shape[0])
            assert filtered == bool((rem >= 1).any() or (rem <= -1).any())
            assert filtered == (c != 2), "case 2 is the no-filter branch, every other case filters"
            if c != 1:
                gap = np.abs(np.abs(rem.astype(np.float64)) - 1.0)
                assert (gap > ar.remap_bound(xy, rot4[0], t2[0])).all(), f"case {c} {s}: a coordinate on the knife edge"
            out[f"c{c}_{s}_xys"], out[f"c{c}_{s}_pos"], out[f"c{c}_{s}_remapped"] = xy, pos, rem
            out[f"c{c}_{s}_candidates"], out[f"c{c}_{s}_filtered"] = cand.astype(np.int64), np.array(filtered)
            out[f"c{c}_{s}_sample_xys"], out[f"c{c}_{s}_sample_pos"] = samp_xy[0].numpy(), samp_pos[0].numpy()
    _save("ref_augment.npz", out)


if __name__ == "__main__":
    main()
