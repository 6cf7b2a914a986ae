"""Farthest-point sampling and point-cloud normals on the device, with pytorch3d's call shapes.

genFeat.py:199-201 thins the key candidates with pytorch3d.ops.sample_farthest_points(fullNegVec, K=80000) on the CPU;
sample_farthest_points below keeps that signature and return order, so the script works with the import line changed.
The sampling is isr_fps_sample (csrc/fps.hpp states the rule: f32 squared distances, the lowest index wins a tie), a
function of (points, lengths, start, K) only.

generateCors.py:211 calls pytorch3d.ops.estimate_pointcloud_normals(fv, neighborhood_size=400);
estimate_pointcloud_normals and estimate_pointcloud_local_coord_frames below keep pytorch3d's names and signatures.  They
are ops.knn of the cloud against itself and ops.local_frames (include/isr_knn.h states both rules).  What pytorch3d does is
restated FROM MEMORY, the library being unavailable to compare against: the covariance divided by the neighbourhood size,
the smallest eigenvalue's vector as the normal, the sign rule and the refusal of neighborhood_size >= N are unpinned.  One
known difference: pytorch3d centres the cloud and works in f32; here the covariance is formed in f64 about each
neighbourhood's own mean, and the results are rounded to f32 at the end.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._capi import require_cuda


def sample_farthest_points(points: torch.Tensor, lengths=None, K=50, random_start_point: bool = False,
                           check_finite: bool = True):
    """points (B,M,3) on the device, lengths (B,) or None, K an int -> (sampled (B,K,3), idx (B,K) int64).
    Clouds shorter than K are padded: idx -1 and sampled rows of zeros.  random_start_point=True draws every cloud's first
    index from torch's CPU generator (torch.manual_seed), otherwise it is 0.  check_finite (one synchronise) refuses
    non-finite coordinates among the first lengths[b] points, which the sampling takes as a precondition."""
    if not isinstance(K, int) or isinstance(K, bool):
        raise ValueError("sample_farthest_points: K must be one int for every cloud (a list of K values is not supported)")
    require_cuda(points)
    if points.ndim != 3 or points.shape[2] != 3:
        raise ValueError(f"sample_farthest_points: points must be (B,M,3), got {tuple(points.shape)}")
    B, M = points.shape[0], points.shape[1]
    lens = None
    if lengths is not None:
        lens = torch.as_tensor(lengths).detach().cpu().to(torch.int64).reshape(-1)
        if lens.numel() != B:
            raise ValueError(f"sample_farthest_points: lengths has {lens.numel()} entries for {B} clouds")
    if check_finite:
        fin = torch.isfinite(points).all(dim=2)
        if lens is not None:
            fin = fin | (torch.arange(M, device=points.device)[None, :] >= lens.to(points.device)[:, None])
        if not bool(fin.all()):
            raise ValueError("sample_farthest_points: non-finite coordinates (finite points are a precondition)")
    start = None
    if random_start_point:
        hi = lens if lens is not None else torch.full((B,), M, dtype=torch.int64)
        start = (torch.rand(B, dtype=torch.float64) * hi.to(torch.float64)).to(torch.int64).clamp_(max=hi - 1)
    idx = ops.fps_sample(points, K, lengths=lens, start=start).to(torch.int64)
    valid = idx >= 0
    sampled = torch.gather(points, 1, idx.clamp(min=0)[..., None].expand(B, K, 3))
    sampled = torch.where(valid[..., None], sampled, torch.zeros((), dtype=points.dtype, device=points.device))
    return sampled, idx


def thin_keys(pts: torch.Tensor, feats: torch.Tensor, n: int):
    """The first n of the farthest-point order of pts (N,3) -> (pts[sel], feats[sel], sel int64): an evenly spread subset of
    a key set (n <= N), instead of a random one."""
    if pts.ndim != 2 or pts.shape[1] != 3 or feats.shape[0] != pts.shape[0]:
        raise ValueError(f"thin_keys: pts {tuple(pts.shape)} and feats {tuple(feats.shape)}")
    if not 1 <= int(n) <= pts.shape[0]:
        raise ValueError(f"thin_keys: n = {n} outside 1..{pts.shape[0]}")
    sel = ops.fps_sample(pts, int(n)).to(torch.int64)
    return pts[sel], feats[sel], sel


def estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size: int = 50, disambiguate_directions: bool = True,
                                           host: bool = False):
    """pointclouds (N,3) or (B,N,3) on the device -> (curvatures (..,N,3) ascending, local_coord_frames (..,N,3,3), columns =
    eigenvectors, column 0 the normal), f32 on the input's device; one ops.knn + ops.local_frames per cloud.
    neighborhood_size >= N raises ValueError, as pytorch3d does.  host=True takes NumPy arrays through the _host entries and
    returns NumPy arrays: the tests' reference, never chosen silently."""
    K = int(neighborhood_size)
    single = pointclouds.ndim == 2
    clouds = pointclouds[None] if single else pointclouds
    if clouds.ndim != 3 or clouds.shape[2] != 3:
        raise ValueError(f"estimate_pointcloud_local_coord_frames: pointclouds must be (N,3) or (B,N,3), got "
                         f"{tuple(pointclouds.shape)}")
    if K < 1 or K >= clouds.shape[1]:
        raise ValueError(f"estimate_pointcloud_local_coord_frames: neighborhood_size = {K} must be in 1..N - 1 = "
                         f"{clouds.shape[1] - 1}")
    curvs, frames = [], []
    for cloud in clouds:
        if host:
            cloud = np.ascontiguousarray(cloud, np.float32)
            c, f = ops.local_frames_host(cloud, ops.knn_host(cloud, cloud, K, want_d2=False)[0], disambiguate_directions)
            c, f = c.astype(np.float32), f.astype(np.float32)
        else:
            c, f = ops.local_frames(cloud, ops.knn(cloud, cloud, K, want_d2=False)[0], disambiguate_directions)
            c, f = c.to(torch.float32), f.to(torch.float32)
        curvs.append(c)
        frames.append(f)
    if single:
        return curvs[0], frames[0]
    return (np.stack(curvs), np.stack(frames)) if host else (torch.stack(curvs), torch.stack(frames))


def estimate_pointcloud_normals(pointclouds, neighborhood_size: int = 50, disambiguate_directions: bool = True,
                                host: bool = False):
    """pointclouds (N,3) or (B,N,3) -> normals of the same shape, f32: column 0 of
    estimate_pointcloud_local_coord_frames(...)[1], the eigenvector of the smallest eigenvalue."""
    return estimate_pointcloud_local_coord_frames(pointclouds, neighborhood_size, disambiguate_directions, host)[1][..., 0]
