"""Shared by the back-march, radius-count and correspondence tests (not a test module): NumPy restatements of
csrc/field_density.hpp's march_ray_back and of csrc/radius_count.hpp's count, the reference's flipped march as torch calls,
ray and cloud fixtures, and the host restatement of correspondences.view_correspondences."""
import numpy as np
import torch

from tests import density_ref as dr

f32, f64 = np.float32, np.float64


def march_back(lengths, rho, threshold):
    """csrc/field_density.hpp's march_ray_back, one ray and one f32 operation at a time -> (weights, depth, hit)."""
    lengths, rho = np.asarray(lengths, f32), np.asarray(rho, f32)
    N, P = lengths.shape
    wts, depth, hit = np.zeros((N, P), f32), np.zeros(N, f32), np.zeros(N, np.int32)
    one = f32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            absorb = one
            for k in range(P - 1, -1, -1):
                if threshold >= 0:
                    c = one if rho[n, k] > f32(threshold) else f32(0.0)
                else:
                    c = rho[n, k]
                wts[n, k] = f32(c * absorb)
                absorb = f32(absorb * f32(one - c))
            for k in range(P):
                v = f32(lengths[n, k] * wts[n, k])
                if k == 0:
                    m = v
                elif not np.isnan(m) and (np.isnan(v) or v > m):
                    m = v
            depth[n] = m
            hit[n] = int(np.any(wts[n] != 0))
    return wts, depth, hit


def torch_march_back(rho, lengths, threshold, eps=1e-10):
    """prenBack.py:365-381's second half as framework calls (the threshold an argument, where the reference writes 0.05):
    weights2 = rho * flip(shifted_cumprod((1 + eps) - flip(rho))) and the caller's depth (generateCors.py:334)."""
    rho = rho.clone()
    if threshold >= 0:
        c1 = rho * 0
        c1[torch.where(rho > threshold)] = 1
        rho = c1
    cp = torch.cumprod((1.0 + eps) - rho.flip(-1), dim=-1)
    absorption2 = torch.cat([torch.ones_like(cp[..., :1]), cp[..., :-1]], dim=-1)
    weights2 = rho * absorption2.flip(-1)
    return weights2, torch.max(lengths * weights2, dim=-1)[0]


def rays(R, P, seed):
    """tests/test_gpu_density.py's rays: origins in the box, unit directions, sorted lengths in [0, 1.5]."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.5, 0.5, (R, 3)).astype(f32)
    d = rng.normal(size=(R, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ln = np.sort(rng.uniform(0.0, 1.5, (R, P)).astype(f32), axis=1)
    return o, d, ln


def brute_count(pts, radius, cap=0):
    """csrc/radius_count.hpp's rule over every pair: d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) <= r * r in f32."""
    p = np.asarray(pts, f32)
    r = f32(radius)
    r2 = f32(r * r)
    out = np.zeros(len(p), np.int32)
    for i in range(len(p)):
        d = (p - p[i]).astype(f32)
        d2 = dr.fma32(d[:, 2], d[:, 2], dr.fma32(d[:, 1], d[:, 1], (d[:, 0] * d[:, 0]).astype(f32)))
        out[i] = int((d2 <= r2).sum())
    return np.minimum(out, cap) if cap > 0 else out


def nearest_f64(points, verts):
    """(index of the nearest vertex, distance) in f64, the lowest index on ties."""
    p, v = np.asarray(points, f64), np.asarray(verts, f64)
    idx = np.zeros(len(p), np.int64)
    dist = np.zeros(len(p), f64)
    for i in range(0, len(p), 256):
        d = np.linalg.norm(p[i:i + 256, None, :] - v[None, :, :], axis=2)
        idx[i:i + 256] = d.argmin(axis=1)
        dist[i:i + 256] = d.min(axis=1)
    return idx, dist


def norm3(v):
    """torch.norm(v, dim=-1) of f32 triples on the CPU (generateCors.py:326), bit for bit: sqrt(fmaf(z, z, fmaf(y, y, x x)))."""
    v = np.asarray(v, f32)
    return np.sqrt(dr.fma32(v[..., 2], v[..., 2], dr.fma32(v[..., 1], v[..., 1], (v[..., 0] * v[..., 0]).astype(f32)))).astype(f32)


def back_rays(o1, ln1, back_scale=3.0):
    """generateCors.py:323-327 in f32 NumPy: -(o / ||o||) and (lengths - lengths[:, :1]) / back_scale, a true f32 division."""
    o1, ln1 = np.asarray(o1, f32), np.asarray(ln1, f32)
    return (-(o1 / norm3(o1)[:, None])).astype(f32), ((ln1 - ln1[:, :1]) / f32(back_scale)).astype(f32)


def view_host(field, o, d, ln, xys, verts, threshold=0.2, back_threshold=0.05, max_dist=0.1, back_scale=3.0):
    """correspondences.view_correspondences from the host calls: march_host, an f64 nearest vertex, the back rays in f32
    NumPy.  -> dict with the six fields (batch dimension 1) and the two distance arrays the filters compared."""
    o, d, ln, xys = (np.asarray(a, f32) for a in (o, d, ln, xys))
    front = field.march_host(o, d, ln, threshold)
    _, dist1 = nearest_f64(front["points"], verts)
    idx1 = np.where(dist1 < max_dist)[0]
    pos = front["points"][idx1]
    o1 = o[idx1]
    bdir, bln = back_rays(o1, ln[idx1], back_scale)
    if len(idx1):
        back = field.march_host(pos, bdir, bln, back_threshold, direction="back")["points"]
        _, dist2 = nearest_f64(back, verts)
    else:
        back, dist2 = np.zeros((0, 3), f32), np.zeros(0)
    idx2 = np.where(dist2 < max_dist)[0]
    return dict(xys=xys[idx1][None], pos_vec=pos[None], pos_vec_back=back[idx2][None], xys_back=xys[idx1][idx2][None],
                idx1=idx1, idx2=idx2, dist1=dist1, dist2=dist2, back_all=back, back_dirs=bdir, back_lengths=bln)


def view_rays(n_side=16, P=24, seed=0):
    """An n_side x n_side bundle aimed at the box from a point outside it: the correspondence tests' view."""
    rng = np.random.default_rng(seed)
    eye = np.array([0.3, -0.4, 2.6], f32)
    u = np.linspace(-0.9, 0.9, n_side).astype(f32)
    gx, gy = np.meshgrid(u, u, indexing="xy")
    target = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3) + rng.uniform(-0.02, 0.02, (n_side * n_side, 3)).astype(f32)
    d = target - eye
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    o = np.tile(eye, (len(d), 1))
    ln = np.tile(np.linspace(1.7, 3.6, P).astype(f32), (len(d), 1))
    xys = np.stack([gx, gy], -1).reshape(-1, 2).astype(f32)
    return o, d, ln, xys


def clouds():
    """name -> (points, radius): the radius-count tests' shapes."""
    rng = np.random.default_rng(5)
    three = np.concatenate([rng.normal(c, 0.05, (n, 3)) for c, n in (((0, 0, 0), 400), ((0.3, 0.1, -0.2), 350),
                                                                     ((-0.4, 0.5, 0.2), 250))]).astype(f32)
    dup = rng.uniform(-0.2, 0.2, (40, 3)).astype(f32)
    far = np.concatenate([rng.normal(0, 0.02, (60, 3)), rng.normal(0, 0.02, (60, 3)) + 1000.0]).astype(f32)
    return {
        "one point": (np.array([[0.25, -1.0, 3.0]], f32), 0.05),
        "two points at exactly r": (np.array([[2, 3, 4], [3, 3, 4]], f32), 1.0),          # d2 == r2 == 1: counted
        "two points past r": (np.array([[2, 3, 4], [3, 3, 5]], f32), 1.0),
        "duplicated points": (np.concatenate([dup, dup[:17], dup[:5]]), 0.1),
        "all identical": (np.tile(np.array([[0.1, 0.2, 0.3]], f32), (33, 1)), 0.05),
        "three clusters": (three, 0.05),
        "box past 2^21 cells": (far, 0.01),                                                 # (1000 / 0.01)^3 cells of size r
        "integer lattice": (np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32), 1.0),
    }
