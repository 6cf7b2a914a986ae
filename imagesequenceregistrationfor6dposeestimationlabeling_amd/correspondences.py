"""view_correspondences: one view of generateCors.py's loop (generateCors.py:250-361) on the device.

generateCors.py extracts the density field's mesh, removes its radius outliers, and then for every training view marches the
view's rays to the front surface, keeps the rays that end near the mesh, shoots a second ray from each surface point towards
the centre, takes the point where that ray LEAVES the surface (the march from the far end, prenBack.py:378-381), keeps the
ones near the mesh again, and saves the four tensors augment.getNerfSamples loads (augment.py:639-702).  The functions here
restate those steps in that order; formats.save_view_correspondences writes the result.  The ray sampler stays the caller's
(pytorch3d's camera conventions are not restated here): `rays` is whatever bundle it made.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from ._capi import require_cuda


@dataclass
class ViewCorrespondences:
    """On the device; n1 rays passed the front filter, n2 of them the back filter."""
    xys: torch.Tensor             # (1, n1, 2)  sampled_rays.xys[:, idx1]            -> <size>_sampledRayxys
    pos_vec: torch.Tensor         # (1, n1, 3)  front surface points                 -> <size>_posVec
    pos_vec_back: torch.Tensor    # (1, n2, 3)  exit points                          -> <size>_posVecBack
    xys_back: torch.Tensor        # (1, n2, 2)  xys of the rays that kept their exit -> <size>_sampledRayBackxys
    idx1: torch.Tensor            # (n1,) int64 into the bundle's rays
    idx2: torch.Tensor            # (n2,) int64 into the n1 kept rays


def clean_mesh_vertices(verts, nb_points: int = 20, radius: float = 0.05):
    """generateCors.py:254-259: the vertices that have more than nb_points vertices within `radius`, themselves included
    (ops.radius_outlier_mask, which states what is known of Open3D's rule and that it is unpinned) -> (verts[ind], ind).
    verts (V,3): a device tensor gives device results (ind int64); a NumPy array is counted on device 0 in f32 and gives
    NumPy results, the kept rows in the array's own dtype."""
    if isinstance(verts, torch.Tensor):
        keep = ops.radius_outlier_mask(verts, nb_points, radius)
        ind = torch.nonzero(keep).reshape(-1)
        return verts[ind], ind
    v = np.asarray(verts)
    dev = torch.device("cuda", torch.cuda.current_device())
    keep = ops.radius_outlier_mask(torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev), nb_points, radius)
    ind = np.nonzero(keep.cpu().numpy())[0]
    return v[ind], ind


def subsampled_normals(mesh_verts, K: int = 1000, neighborhood_size: int = 400, host: bool = False):
    """generateCors.py:205-212: the mesh vertices as f32, reduced to K points by farthest-point sampling from index 0
    (sampling.sample_farthest_points(v[None], K=K)[1][0], pytorch3d's default start), and the NEGATED
    sampling.estimate_pointcloud_normals(subvert, neighborhood_size) of that subset -> (subvert (K,3) f32, subnormal (K,3)
    f32): what formats.save_subsampled_normals writes.  mesh_verts (V,3): a device tensor gives device tensors; a NumPy array
    is worked on device 0 and gives NumPy arrays.  Fewer than K vertices, or neighborhood_size >= K, raises ValueError.
    host=True runs the same steps through the _host entries on a NumPy array (the tests' reference)."""
    from . import sampling
    K, nb = int(K), int(neighborhood_size)
    if mesh_verts.ndim != 2 or mesh_verts.shape[1] != 3:
        raise ValueError(f"subsampled_normals: mesh_verts must be (V,3), got {tuple(mesh_verts.shape)}")
    if K < 1 or mesh_verts.shape[0] < K:
        raise ValueError(f"subsampled_normals: {mesh_verts.shape[0]} vertices, K = {K}")
    if nb < 1 or nb >= K:
        raise ValueError(f"subsampled_normals: neighborhood_size = {nb} must be in 1..K - 1 = {K - 1}")
    if host:
        v = np.ascontiguousarray(mesh_verts, np.float32)
        sub = v[ops.fps_sample_host(v, K)[0].astype(np.int64)]
        return sub, -sampling.estimate_pointcloud_normals(sub, nb, host=True)
    as_numpy = not isinstance(mesh_verts, torch.Tensor)
    if as_numpy:
        dev = torch.device("cuda", torch.cuda.current_device())
        mesh_verts = torch.from_numpy(np.ascontiguousarray(mesh_verts, np.float32)).to(dev)
    v = mesh_verts.to(torch.float32)
    sub = v[sampling.sample_farthest_points(v[None], K=K)[1][0]]
    normal = -sampling.estimate_pointcloud_normals(sub, nb)
    return (sub.cpu().numpy(), normal.cpu().numpy()) if as_numpy else (sub, normal)


def near_mesh(points: torch.Tensor, verts64: np.ndarray, verts32: torch.Tensor, max_dist: float) -> torch.Tensor:
    """Indices of the points within max_dist of their nearest mesh vertex, as key_export.export_keys step 3 finds it: the
    vertex by ops.nn_batched (an f32 search, the lowest index on ties), the distance in f64 to that vertex as the mesh holds
    it.  points (n,3) f32 on the device -> (m,) int64 on the device."""
    if points.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=points.device)
    nearest = ops.nn_batched(points, verts32, want_idx=True).nn_idx[0].to(torch.int64).cpu().numpy()
    dist = np.linalg.norm(points.cpu().numpy().astype(np.float64) - verts64[nearest], axis=1)
    return torch.from_numpy(np.where(dist < max_dist)[0]).to(points.device)


def _fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fmaf(a, b, c) of f32 tensors, exactly, from f64 operations: the f64 product of two f32 is exact; the f64 sum is rounded
    to odd (TwoSum tells whether it was inexact), and rounding that to f32 is then a single rounding (53 >= 2 * 24 + 2)."""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(torch.int64)
    fix = torch.isfinite(s) & (err != 0) & ((bits & 1) == 0)
    step = torch.where((err > 0) == (s > 0), 1, -1)
    return torch.where(fix, bits + step, bits).view(torch.float64).to(torch.float32)


def norm3_f32(v: torch.Tensor) -> torch.Tensor:
    """torch.norm(v, dim=-1) of f32 triples as torch's CPU kernel takes it, bit for bit, on any device: the squares are
    accumulated x, y, z in f32 with each product contracted into the sum, sqrt(fmaf(z, z, fmaf(y, y, x * x))) (measured:
    equal on 200 000 random triples, where the uncontracted x x + y y + z z differs in one row of nine).  The square root is
    taken in f64 and rounded, which is the correctly rounded f32 root.  v (..., 3) f32 -> (...) f32."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return torch.sqrt(_fma32(z, z, _fma32(y, y, x * x)).double()).to(torch.float32)


def back_rays(origins: torch.Tensor, lengths: torch.Tensor, back_scale: float = 3.0):
    """generateCors.py:323-327 on the kept rays, f32 on their device: origins (n, 3), lengths (n, P) -> (directions (n, 3),
    lengths (n, P)) of the rays shot back from the surface points: -(o / ||o||) with ||o|| = norm3_f32(o), the reference's
    torch.norm on CPU tensors bit for bit, and (lengths - lengths[:, :1]) / back_scale."""
    directions = -(origins / norm3_f32(origins)[:, None])
    # the reference takes this quotient on CPU tensors (generateCors.py:316-323 moves the bundle to the host first): a true
    # f32 division.  On the device torch divides by a host scalar as a multiplication by its reciprocal, another rounding;
    # a 0-d device tensor as the divisor keeps the division
    scale = torch.tensor(float(back_scale), dtype=torch.float32, device=lengths.device)
    return directions, (lengths - lengths[:, :1]) / scale


def view_correspondences(field, rays, mesh_verts, threshold: float = 0.2, back_threshold: float = 0.05, max_dist: float = 0.1,
                         back_scale: float = 3.0) -> ViewCorrespondences:
    """generateCors.py:299-349 for one view.  field: a fields.DensityField; rays: any object with .origins, .directions
    (1, n, 3), .lengths (1, n, P) and .xys (1, n, 2) on the device; mesh_verts (V, 3): the cleaned mesh vertices
    (clean_mesh_vertices), NumPy or a tensor.
      1. posVec: the front march at `threshold` (:306);
      2. idx1: the rays whose posVec is within max_dist of its nearest mesh vertex (:308-309, near_mesh);
      3. the back rays of the kept rays (:323-329, back_rays), f32 on the device: origin posVec, direction -(o / ||o||) of
         the RAY's origin with ||o|| = norm3_f32(o), the reference's torch.norm on CPU tensors (:326) bit for bit, lengths
         (lengths - lengths[..., :1]) / back_scale;
      4. posVecBack: the march of the back rays from their far end at back_threshold (:331-334): the last sample above it.
         back_threshold is 0.05 because prenBack.py:367 compares against the literal 0.05 — it ignores the threshold = 0.2
         the script sets at generateCors.py:182 for the front march;
      5. idx2: the same mesh-distance filter on posVecBack (:338-341)."""
    dev = require_cuda(rays.origins, rays.directions, rays.lengths, rays.xys)
    if rays.origins.ndim != 3 or rays.origins.shape[0] != 1 or rays.xys.shape[:2] != rays.origins.shape[:2]:
        raise ValueError(f"view_correspondences: origins {tuple(rays.origins.shape)}, xys {tuple(rays.xys.shape)}: expected "
                         "(1, n, 3) and (1, n, 2)")
    v64 = np.ascontiguousarray(mesh_verts.detach().cpu().numpy() if isinstance(mesh_verts, torch.Tensor) else mesh_verts,
                               np.float64)
    if v64.ndim != 2 or v64.shape[1] != 3 or len(v64) == 0:
        raise ValueError(f"view_correspondences: mesh_verts {v64.shape} must be (V, 3) with V >= 1")
    v32 = torch.from_numpy(v64.astype(np.float32)).to(dev)
    f32 = lambda t: t.to(torch.float32)
    o, ln, xys = f32(rays.origins)[0], f32(rays.lengths)[0], rays.xys[0]

    pos, _, _ = field.surface_points(rays.origins, rays.directions, rays.lengths, threshold=threshold)
    pos = pos[0]
    idx1 = near_mesh(pos.contiguous(), v64, v32, max_dist)
    pos, o1, ln1, xys1 = pos[idx1].contiguous(), o[idx1], ln[idx1], xys[idx1]

    back_dirs, back_lengths = back_rays(o1, ln1, back_scale)
    if pos.shape[0]:
        back, _, _ = field.surface_points(pos, back_dirs, back_lengths, threshold=back_threshold, direction="back")
    else:
        back = pos
    idx2 = near_mesh(back.contiguous(), v64, v32, max_dist)
    return ViewCorrespondences(xys=xys1[None], pos_vec=pos[None], pos_vec_back=back[idx2][None], xys_back=xys1[idx2][None],
                               idx1=idx1, idx2=idx2)
