#!/usr/bin/env python3
"""Generates tests/golden/ref_back_march.npz by EXECUTING THE REFERENCE'S OWN STATEMENTS prenBack.py:362-385 (the body of
EmissionAbsorptionRaymarcher... .forward after its input checks): weights and weights2 of the ray marcher that
generateCors.py:332-334 calls, in thresholdMode (the literal 0.05 of prenBack.py:367) and in plain emission-absorption.

Runs in the build container only (it reads the reference checkout).  As make_golden_from_reference.py does, nothing of the
reference is imported or stored: the file is parsed with `ast`, the statements of the line range are compiled and executed
(its `return` dropped: the values are read from the namespace), and only DATA is written — the inputs and what the
reference's statements made of them.

pytorch3d is absent, so `_shifted_cumprod` is supplied here FROM MEMORY of pytorch3d/renderer/implicit/raymarching.py:
cat(ones_like(x[..., :shift]), cumprod(x)[..., :-shift]).  It is not the reference's text and not pinned.

Run from the repo root:  python tests/golden/make_ref_back_march.py
"""
import ast
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_golden_from_reference import OUT, _stmts_in, _tree      # noqa: E402


def _shifted_cumprod(x, shift=1):
    x_cumprod = torch.cumprod(x, dim=-1)
    return torch.cat([torch.ones_like(x_cumprod[..., :shift]), x_cumprod[..., :-shift]], dim=-1)


def marcher_code():
    out = []
    _stmts_in(_tree("prenBack.py").body, 362, 385, out)
    out = [s for s in out if not isinstance(s, ast.Return)]
    text = "\n".join(ast.unparse(s) for s in out)
    for needle in ("weights2", "absorption2", "rays_densities > 0.05", ".flip(-1)"):
        assert needle in text, f"prenBack.py:362-385: expected `{needle}` in the extracted statements"
    return compile(ast.Module(body=out, type_ignores=[]), "prenBack.py:362-385", "exec")


def main():
    rng = np.random.default_rng(20261018)
    code = marcher_code()
    R, P = 24, 20
    rho = rng.uniform(0.0, 0.12, (1, R, P)).astype(np.float32)
    rho[0, 0] = 0.01                                     # no sample above 0.05
    rho[0, 1] = 0.5                                      # every sample above it
    rho[0, 2, :-1], rho[0, 2, -1] = 0.01, 0.5            # only the last
    rho[0, 3, 1:], rho[0, 3, 0] = 0.01, 0.5              # only the first
    rho[0, 4] = 0.05                                     # exactly the threshold: not above
    lengths = np.sort(rng.uniform(0.0, 1.5, (1, R, P)).astype(np.float32), axis=-1)
    lengths[0, 5] = -lengths[0, 5]
    lengths[0, 6, 0] = 0.0
    out = dict(rho=rho, lengths=lengths)
    for mode, tag in ((True, "threshold"), (False, "soft")):
        ns = {"torch": torch, "_shifted_cumprod": _shifted_cumprod, "eps": 1e-10,
              "self": types.SimpleNamespace(thresholdMode=mode, surface_thickness=1),
              "rays_densities": torch.from_numpy(rho)[..., None].clone(),
              "rays_features": torch.zeros((1, R, P, 1))}
        exec(code, ns)
        w, w2 = ns["weights"], ns["weights2"]
        cat = torch.cat([w, w2], dim=-1)
        tl = torch.from_numpy(lengths)
        out[f"{tag}_weights"] = cat.numpy()                                                         # prenBack.py:385
        out[f"{tag}_depth_back"] = torch.max(tl * cat[:, :, P:], dim=-1)[0].numpy()                # generateCors.py:334
        out[f"{tag}_depth_front"] = torch.max(tl * cat[:, :, 0:P], dim=-1)[0].numpy()              # generateCors.py:306
    np.savez_compressed(OUT / "ref_back_march.npz", **out)
    print("wrote", OUT / "ref_back_march.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
