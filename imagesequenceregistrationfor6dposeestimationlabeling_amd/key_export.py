"""export_keys: from key candidates to the three arrays the pose stages load (genFeat.py:201-228).

genFeat.py collects candidate surface points from the trained field's rays, thins them by farthest-point sampling, keeps the
ones inside the volume and close to the extracted mesh, looks up each one's mesh normal and key descriptor, and scales the
points to the object's units.  export_keys restates those steps in that order on the device; formats.save_model writes the
result where formats.load_model reads it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._capi import require_cuda


def export_keys(candidates: torch.Tensor, mesh, field, diameter: float, K: int = 80000, box: float = 1.2,
                max_dist: float = 0.05, diam_scaling: float = 1.8):
    """candidates (M,3) on the device, in the field's coordinates; mesh a render.Mesh in the same coordinates; field any
    object with batched_customForward(points) -> (..., D + 1) (fields.KeyField is the intended one) ->
    (vert_scaled (N,3) f32, feats (N,D) f32, normals (N,3) f64, kept (N,) int64 into candidates), NumPy, rows in FPS order.
      1. farthest-point sampling to K from candidate 0 (genFeat.py:201-202); with M < K every candidate, in FPS order;
      2. keep max|coord| < box (:204);
      3. the nearest mesh vertex by ops.nn_batched (an f32 search, the lowest index on ties), and keep dist < max_dist
         (:212-216), the distance taken in f64 between the point and that vertex as the mesh holds it;
      4. normals = mesh.vertex_normals()[nearest] (:209-210, :217);
      5. feats = field.batched_customForward(points)[..., :-1] (:219-222, :224);
      6. vert_scaled = points * f32(diameter / diam_scaling) (:223)."""
    dev = require_cuda(candidates)
    if candidates.ndim != 2 or candidates.shape[1] != 3 or candidates.shape[0] < 1:
        raise ValueError(f"export_keys: candidates must be (M,3) with M >= 1, got {tuple(candidates.shape)}")
    if int(K) < 1:
        raise ValueError(f"export_keys: K = {K}")
    cand = candidates.to(torch.float32).contiguous()
    order = ops.fps_sample(cand, min(int(K), cand.shape[0])).to(torch.int64)
    pts = cand[order]
    inbox = pts.abs().amax(dim=1) < box
    order, pts = order[inbox], pts[inbox]
    verts = np.asarray(mesh.mesh.vertices, np.float64)
    normals, nearest = np.zeros((0, 3)), np.zeros(0, np.int64)
    if pts.shape[0]:
        if len(verts) == 0:
            raise ValueError("export_keys: the mesh has no vertex")
        nn = ops.nn_batched(pts, torch.from_numpy(verts.astype(np.float32)).to(dev), want_idx=True)
        nearest = nn.nn_idx[0].to(torch.int64).cpu().numpy()
        dist = np.linalg.norm(pts.cpu().numpy().astype(np.float64) - verts[nearest], axis=1)
        close = dist < max_dist
        nearest = nearest[close]
        close = torch.from_numpy(close).to(dev)
        order, pts = order[close], pts[close].contiguous()
        normals = mesh.vertex_normals()[nearest]
    feats = field.batched_customForward(pts)[..., :-1]
    scaled = pts.cpu().numpy() * np.float32(diameter / diam_scaling)
    return scaled, feats.detach().to(torch.float32).cpu().numpy(), normals, order.cpu().numpy()


def extract_mesh(density_field, threshold: float = 0.05, res: int = 128, coords: str = "reference"):
    """genFeat.py:206-209: the density field's iso-surface as a render.Mesh, export_keys' `mesh`
    (fields.DensityField.batched_forward_forPC explains `coords`), so that
    export_keys(candidates, extract_mesh(df), key_field, diameter) is the whole of genFeat.py:201-224."""
    from .render import Mesh
    verts, tris = density_field.batched_forward_forPC(threshold=threshold, res=res, coords=coords)
    return Mesh(verts, tris)


def collect_candidates(field, bundles, threshold: float = 0.2) -> torch.Tensor:
    """genFeat.py:191-198: the surface point of every ray of every bundle (any objects with .origins, .directions (..., 3) and
    .lengths (..., P); field a fields.DensityField), rays whose point did not leave the origin dropped (the reference's
    `where(norm(point - origin))`: no hit, or a hit at depth 0), concatenated on the device in bundle order, rays in their
    own order -> (M, 3) f32: export_keys' `candidates`."""
    parts = []
    for rb in bundles:
        pts, _, _ = field.surface_points(rb.origins, rb.directions, rb.lengths, threshold=threshold)
        pts = pts.reshape(-1, 3)
        moved = torch.linalg.vector_norm(pts - rb.origins.to(torch.float32).reshape(-1, 3), dim=-1) != 0
        parts.append(pts[moved])
    if not parts:
        raise ValueError("collect_candidates: no bundle")
    return torch.cat(parts).contiguous()
