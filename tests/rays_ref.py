"""Restatements for the ray tests (test infrastructure): BOP-style cameras converted as generateCors.py:98-102 does, the
torch.linspace / meshgrid grid, the literal grid_sample expression of nutil.py:188-193 with torch.where, the f64 plane-1 /
plane-2 unprojection through 4x4 matrices, and the derived bounds of the geometry checks.

`python -m tests.rays_ref` measures the geometry checks on the host build and writes profiles/rays_parity.json."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
EPS = 2.0 ** -24

# ---- the cameras of the geometry checks and what bounds their numbers
T_MAX = 4.6          # |t| <= sqrt(0.5^2 + 0.5^2 + 4.5^2) < 4.6, and every camera depth Z <= 4.5 + 0.5 < T_MAX + 0.5
Z_MAX = 5.0
C_SUM = 2.2          # |c_x| + |c_y| + 1 with |c_x|, |c_y| <= 0.6: |x - px| <= 2.6 over fx >= 4.4 (f >= 500 px at s <= 224)
# Roundings (each at most 2^-24 of the magnitude it acts on) behind one component of an output:
#   origin_i = dot3(-T, R_i):  3 (T to f32) + 6 (R to f32: R^T differs from R^-1 by at most 2 * 2^-24 per entry, three entries)
#                              + 3 (the product and the two fmaf)                                   = 12 at magnitude <= T_MAX
#   direction_i = dot3(c, R_i): c_x and c_y each carry 8 (xy to f32; px: its own rounding, p - W/2, / s; x - px; fx: its own
#                              rounding, / s; the division), at magnitudes below C_SUM               = 16
#                              + 6 (R to f32) + 3 (the product and the two fmaf)                     = 25 at magnitude <= C_SUM
BOUND_ORIGIN = 12 * EPS * T_MAX
BOUND_DIRECTION = 25 * EPS * C_SUM
BOUND_POINT = BOUND_ORIGIN + Z_MAX * BOUND_DIRECTION      # origin + direction * Z_cam against the world point
# grid xy against the NDC of the pixel centre (computed in f64), per unit of range: the end point's rounding (1), the step
# (the other end point's rounding, the subtraction, the division: 3, acting on |step k| <= range since k < W / 2 on either
# branch) and the fmaf (1) make 5; 6 taken
BOUND_PIXEL = 6 * EPS


def rot180z():
    """nutil.rotfromeulernp([0, 0, pi]) without the 1e-16 of sin(pi)."""
    return np.diag([-1.0, -1.0, 1.0])


def random_rotations(rng, B):
    q = rng.normal(size=(B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def bop_cameras(rng, B, H, W):
    """-> dict: OpenCV poses (R_cv, t_cv, K) in f64 with x_cv = R_cv X + t_cv, u = fx x/z + cx, and the arguments of
    rays.PerspectiveCameras after generateCors.py:98-102's two statements (R = R_cv^T rot180, T[0:2] = -T[0:2])."""
    R_cv = random_rotations(rng, B)
    t_cv = np.stack([rng.uniform(-0.5, 0.5, B), rng.uniform(-0.5, 0.5, B), rng.uniform(2.5, 4.5, B)], 1)
    s = min(H, W)
    K = np.zeros((B, 3, 3))
    K[:, 0, 0] = rng.uniform(500, 700, B) * s / 224
    K[:, 1, 1] = K[:, 0, 0] * rng.uniform(0.97, 1.03, B)
    K[:, 0, 2] = W / 2 + rng.uniform(-0.05, 0.05, B) * W
    K[:, 1, 2] = H / 2 + rng.uniform(-0.05, 0.05, B) * H
    K[:, 2, 2] = 1
    R = np.stack([R_cv[a].T.dot(rot180z()) for a in range(B)])
    T = t_cv.copy()
    T[:, 0:2] = -T[:, 0:2]
    return dict(R_cv=R_cv, t_cv=t_cv, K=K, R=R.astype(f32), T=T.astype(f32), focal=np.stack([K[:, 0, 0], K[:, 1, 1]], 1).astype(f32),
                principal=K[:, 0:2, 2].astype(f32), image_size=(H, W))


def ndc_of_pixel(u, v, H, W):
    s = min(H, W)
    return -(u - W / 2) * 2 / s, -(v - H / 2) * 2 / s


def pixel_of_ndc(x, y, H, W):
    s = min(H, W)
    return W / 2 - x * s / 2, H / 2 - y * s / 2


def world_points(cam, b, u, v, Z):
    """The world points that camera b (OpenCV convention, the f32-rounded pose and intrinsics promoted to f64) sees at pixels
    (u, v) and depth Z."""
    R_cv = (cam["R"][b].astype(np.float64) @ rot180z()).T              # back from the converted f32 pose
    t_cv = cam["T"][b].astype(np.float64) * np.array([-1.0, -1.0, 1.0])
    fx, fy = cam["focal"][b].astype(np.float64)
    cx, cy = cam["principal"][b].astype(np.float64)
    x_cv = np.stack([(u - cx) / fx * Z, (v - cy) / fy * Z, Z], -1)
    return (x_cv - t_cv) @ np.linalg.inv(R_cv).T


def unproject_planes_f64(R, T, intr, xy):
    """pytorch3d's rule restated in f64: unproject (x, y) at depths 1 and 2 through the inverse of the 4x4
    world-to-view x projection, direction = plane2 - plane1, origin = plane1 - direction.  R (3,3), T (3,), intr (4,), xy (n,2)."""
    R, T, intr, xy = (np.asarray(a, np.float64) for a in (R, T, intr, xy))
    wv = np.eye(4)
    wv[:3, :3], wv[3, :3] = R, T
    fx, fy, px, py = intr
    Kp = np.array([[fx, 0, px, 0], [0, fy, py, 0], [0, 0, 0, 1], [0, 0, 1, 0]], np.float64)
    inv = np.linalg.inv(wv @ Kp.T)
    planes = []
    for z in (1.0, 2.0):
        h = np.concatenate([xy, np.full((len(xy), 1), 1.0 / z), np.ones((len(xy), 1))], 1) @ inv
        planes.append(h[:, :3] / h[:, 3:4])
    d = planes[1] - planes[0]
    return planes[0] - d, d


def grid_xys(H, W):
    """pytorch3d's NDC grid restated with torch.linspace and meshgrid (CPU, f32): (H, W, 2), [..., 0] = x."""
    if W >= H:
        range_x, range_y = W / H, 1.0
    else:
        range_x, range_y = 1.0, H / W
    hx, hy = range_x / W, range_y / H
    xs = torch.linspace(range_x - hx, -range_x + hx, W, dtype=torch.float32)
    ys = torch.linspace(range_y - hy, -range_y + hy, H, dtype=torch.float32)
    Y, X = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack([X, Y], -1).numpy()


def sample_literal(images, xys):
    """nutil.py:188-196, literally."""
    target_images, sampled_rays_xy = torch.as_tensor(images), torch.as_tensor(xys)
    ba = target_images.shape[0]
    dim = target_images.shape[-1]
    spatial_size = sampled_rays_xy.shape[1:-1]
    images_sampled = torch.nn.functional.grid_sample(
        target_images.permute(0, 3, 1, 2),
        -sampled_rays_xy.view(ba, -1, 1, 2),
        align_corners=True,
        mode='nearest'
    )
    return images_sampled.permute(0, 2, 3, 1).view(ba, *spatial_size, dim).numpy()


def select_literal(mask, bundle):
    """pren.py:231-235: torch.where over the sampled mask, then the four fields indexed by it.  mask (B, mh, mw); bundle: the
    (o, d, lengths, xys) of every ray as (B, n, .) arrays -> (o, d, lengths, xys) of (M, .) and src (M,)."""
    o, d, ln, xy = (torch.as_tensor(a) for a in bundle)
    maskVals = torch.where(torch.as_tensor(sample_literal(mask[..., None], xy.numpy()))[..., 0])
    src = maskVals[0] * xy.shape[1] + maskVals[1]
    return o[maskVals].numpy(), d[maskVals].numpy(), ln[maskVals].numpy(), xy[maskVals].numpy(), src.numpy().astype(np.int32)


def masks(rng, B, mh, mw):
    """name -> (B, mh, mw) f32 masks for the selection tests."""
    checker = ((np.add.outer(np.arange(mh), np.arange(mw)) % 2) == 0).astype(f32)
    out = {"empty": np.zeros((B, mh, mw), f32), "full": np.ones((B, mh, mw), f32), "checker": np.tile(checker, (B, 1, 1)),
           "random": (rng.uniform(size=(B, mh, mw)) < 0.3).astype(f32)}
    nan = out["random"].copy() * f32(0.5)
    nan[rng.uniform(size=nan.shape) < 0.1] = np.nan
    out["holding NaN"] = nan
    if B >= 3:
        hole = out["random"].copy()
        hole[1] = 0                                                  # a camera that keeps nothing between two that keep some
        out["camera 1 keeps nothing"] = hole
    return out


def measure():
    """The geometry checks on the host build: the largest distances, per check."""
    from tests import test_rays_cpu as t
    return {"point_from_ray_max_abs": t.point_error(), "closed_form_vs_f64": dict(zip(("origin_max_abs", "direction_max_abs"), t.closed_form_error())),
            "grid_pixel_max_abs_per_range": t.pixel_error(),
            "bounds": {"BOUND_POINT": BOUND_POINT, "BOUND_ORIGIN": BOUND_ORIGIN, "BOUND_DIRECTION": BOUND_DIRECTION, "BOUND_PIXEL": BOUND_PIXEL},
            "note": "measured on the CPU by python -m tests.rays_ref; the bounds are derived in tests/rays_ref.py, not from these figures"}


if __name__ == "__main__":
    doc = measure()
    (ROOT / "profiles" / "rays_parity.json").write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))
