"""ObjCoordRenderer with the reference's interface (renderer.py:37-117), drawn by HIP kernels instead of OpenGL.

The reference renders the object's visible surface with moderngl on EGL: a (h, w, 4) f32 image of (vertex - offset) / scale
with alpha 1 where the mesh is visible, which refine_pose turns into the visible object coordinates.  This class gives the
same image from isr_render_coords_batch (csrc/render_coords.hip): a triangle rasteriser whose rules — 1/256-pixel snapping,
top-left fill rule, no culling, f32 depth test with the lower face index winning ties, perspective-correct colour — are
stated in csrc/raster.hpp.  Interior pixels are what GL gives; a pixel whose centre lies within a sub-pixel step of an edge
may differ from a particular GL driver, and a face that crosses the near plane is dropped instead of clipped.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


def ritter_sphere(points):
    """Ritter's bounding sphere of points (N,3) -> (centre (3,) f64, radius): two farthest-point passes for the start, then
    grown point by point; the radius is finally raised to the farthest point's distance, so every point is inside."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    y = p[np.argmax(((p - p[0]) ** 2).sum(1))]
    z = p[np.argmax(((p - y) ** 2).sum(1))]
    c, r = (y + z) / 2, float(np.linalg.norm(y - z)) / 2
    while True:
        d = np.sqrt(((p - c) ** 2).sum(1))
        k = int(np.argmax(d))
        if d[k] <= r * (1 + 1e-12) or d[k] == 0:
            break
        r_new = (r + d[k]) / 2
        c = c + (p[k] - c) * ((d[k] - r_new) / d[k])
        r = r_new
    return c, float(max(r, np.sqrt(((p - c) ** 2).sum(1)).max()))


class _TriMesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces


class Mesh:
    """What the renderer needs of the reference's Obj: .mesh.vertices (V,3), .mesh.faces (F,3), .offset (3,), .scale,
    .diameter.  offset and scale default to the centre and radius of Ritter's bounding sphere of the vertices (the reference
    takes trimesh's minimum bounding sphere, which may differ slightly: pass the reference's values to reproduce its
    colours); diameter defaults to twice that radius."""

    def __init__(self, vertices, faces, offset=None, scale=None, diameter=None):
        v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        if len(f) and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError(f"Mesh: face index outside the {len(v)} vertices")
        self.mesh = _TriMesh(v, f)
        if offset is None or scale is None:
            c, r = ritter_sphere(v)
        self.offset = np.asarray(c if offset is None else offset, np.float64).reshape(3)
        self.scale = float(r if scale is None else scale)
        self.diameter = float(2 * self.scale if diameter is None else diameter)

    def vertex_normals(self) -> np.ndarray:
        """(V,3) f64 unit vertex normals: the sum of the adjacent faces' unit normals (right-hand rule over the face's vertex
        order), each weighted by the face's corner angle at the vertex, normalised.  This is what trimesh's default
        Trimesh.vertex_normals computes, which genFeat.py:209-210 saves for the keys (restated from memory of trimesh: it is
        not installed beside this package to compare against).  A zero-area face contributes nothing; a vertex with no face,
        or whose weighted normals cancel, gets (0, 0, 0)."""
        v, f = self.mesh.vertices, self.mesh.faces.astype(np.int64)
        out = np.zeros_like(v)
        if len(f) == 0:
            return out
        p = v[f]                                                  # (F, 3 corners, 3)
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        area2 = np.linalg.norm(n, axis=1)
        ok = area2 > 0
        n[ok] /= area2[ok, None]
        for c in range(3):
            e1, e2 = p[:, (c + 1) % 3] - p[:, c], p[:, (c + 2) % 3] - p[:, c]
            l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
            cos = np.einsum("ij,ij->i", e1[ok], e2[ok]) / (l1[ok] * l2[ok])     # area > 0: both edges have length
            np.add.at(out, f[ok, c], n[ok] * np.arccos(np.clip(cos, -1.0, 1.0))[:, None])
        ln = np.linalg.norm(out, axis=1)
        nz = ln > 0
        out[nz] /= ln[nz, None]
        return out


class ObjCoordRenderer:
    """renderer.py:37-117.  objs[i] has .mesh.vertices, .mesh.faces, .offset, .scale (the reference's Obj, or Mesh above).
    The frame buffer lives on the device (cuda:device_idx) and persists between calls, so render(..., clear=False) draws on
    top of the previous image as the reference's does.  n_calls counts isr_render_coords_batch calls."""

    def __init__(self, objs, w: int, h: int = None, device_idx=0, near=10., far=10000.):
        self.objs = objs
        if h is None:
            h = w
        self.h, self.w = int(h), int(w)
        self.near, self.far = float(near), float(far)
        self.device = torch.device("cuda", device_idx)
        self._meshes = []
        for obj in objs:
            v = torch.from_numpy(np.ascontiguousarray(obj.mesh.vertices, np.float32).reshape(-1, 3)).to(self.device)
            f = torch.from_numpy(np.ascontiguousarray(obj.mesh.faces, np.int32).reshape(-1, 3)).to(self.device)
            o = torch.from_numpy(np.ascontiguousarray(np.asarray(obj.offset, np.float32).reshape(3))).to(self.device)
            self._meshes.append((v, f, o, float(obj.scale)))
        self._words = ops.render_state_words(self.h, self.w)
        self._state = torch.zeros((1, self._words), dtype=torch.float32, device=self.device)
        self.n_calls = 0

    def _cameras(self, Ks, Rs, ts):
        """-> (K (B,9), Rt (B,12)) f64 on the device, one copy."""
        B = len(Rs)
        Ka = np.asarray(Ks, np.float64)
        Ka = np.broadcast_to(Ka, (B, 3, 3)) if Ka.ndim == 2 else Ka.reshape(B, 3, 3)
        both = np.empty((B, 21), np.float64)
        both[:, :9] = Ka.reshape(B, 9)
        for b in range(B):
            both[b, 9:] = np.concatenate([np.asarray(Rs[b], np.float64).reshape(3, 3),
                                          np.asarray(ts[b], np.float64).reshape(3, 1)], axis=1).reshape(12)
        d = torch.from_numpy(both).to(self.device)
        return d[:, :9].contiguous(), d[:, 9:].contiguous()

    def _draw(self, obj_idx, K, Rt, clear, state):
        v, f, o, scale = self._meshes[obj_idx]
        self.n_calls += 1
        return ops.render_coords_batch(v, f, K, Rt, self.h, self.w, o, scale, self.near, self.far, clear, state)

    def read(self):
        n = 4 * self.h * self.w
        return self._state[0, :n].reshape(self.h, self.w, 4).cpu().numpy()

    def read_depth(self):
        """Camera z per pixel, 0 where nothing was drawn (what the reference recovers from the GL depth buffer)."""
        n = self.h * self.w
        return self._state[0, 4 * n:5 * n].reshape(self.h, self.w).cpu().numpy()

    def counters(self):
        """{faces drawn, faces dropped at the near plane, pixels covered} of the frame buffer's last draw."""
        c = self._state[0, 5 * self.h * self.w:].view(torch.int32).cpu().numpy()
        return {"drawn": int(c[0]), "dropped": int(c[1]), "covered": int(c[2])}

    def render(self, obj_idx, K, R, t, clear=True, read=True, read_depth=False):
        """One image into the persistent frame buffer.  K (3,3), R (3,3), t (3,1) or (3,).  Returns the (h,w,4) f32 NumPy
        image (read), or the depth (read_depth), or None."""
        Kd, Rtd = self._cameras(K, [R], [t])
        self._draw(obj_idx, Kd, Rtd, bool(clear), self._state)
        if read_depth:
            return self.read_depth()
        elif read:
            return self.read()
        else:
            return None

    def render_batch(self, obj_idx, Ks, Rs, ts):
        """B images of one object in one call, no host copy: Ks one (3,3) or (B,3,3), Rs B x (3,3), ts B x (3,) or (3,1) ->
        (B,h,w,4) f32 on the device.  Image b is render(obj_idx, Ks[b], Rs[b], ts[b]) bit for bit.  The persistent frame
        buffer of render() is not touched."""
        B = len(Rs)
        if len(ts) != B:
            raise ValueError(f"render_batch: {B} rotations, {len(ts)} translations")
        if B == 0:
            return torch.empty((0, self.h, self.w, 4), dtype=torch.float32, device=self.device)
        Kd, Rtd = self._cameras(Ks, Rs, ts)
        state = self._draw(obj_idx, Kd, Rtd, True, None)
        return state[:, :4 * self.h * self.w].reshape(B, self.h, self.w, 4)

    @staticmethod
    def extract_mask(model_coords_img: np.ndarray):
        """Alpha is 1 where the mesh is visible.  (The reference compares with 255, a leftover from a u8 frame buffer that
        its f4 one never matches; refine_pose tests == 1 itself.)"""
        return model_coords_img[..., 3] == 1

    def denormalize(self, model_coords: np.ndarray, obj_idx: int):
        return model_coords * self.objs[obj_idx].scale + self.objs[obj_idx].offset


def get_emb_vis(emb_img: torch.Tensor, mask: torch.Tensor = None, demean=False) -> torch.Tensor:
    """nutil.get_emb_vis (nutil.py:198-210): an embedding image (..., 3 n) to three channels in [0, 1] for viewing: the
    optional mean over the mask taken off, groups of n channels averaged, pixels off the mask zeroed, scaled by the
    largest magnitude."""
    last = emb_img.shape[-1]
    if demean is True:
        demean = emb_img[mask].view(-1, last).mean(dim=0)
    if demean is not False:
        emb_img = emb_img - demean
    emb_img = emb_img.view(*emb_img.shape[:-1], 3, -1).mean(dim=-1)
    if mask is not None:
        emb_img[~mask] = 0.
    emb_img /= torch.abs(emb_img).max() + 1e-9
    emb_img.mul_(0.5).add_(0.5)
    return emb_img


def normImage(emb_img: torch.Tensor) -> torch.Tensor:
    """nutil.normImage (nutil.py:345-348): in place, the image over its largest magnitude, then halved around 0.5."""
    emb_img /= torch.abs(emb_img).max() + 1e-9
    emb_img.mul_(0.5).add_(0.5)
    return emb_img


def full_render(field, camera, renderer_grid):
    """The tensor half of nutil.show_full_render1 (nutil.py:233-246): renderer_grid(cameras=camera,
    volumetric_function=field.batched_forward), the first image split into (rendered_image (H, W, F),
    rendered_silhouette (H, W, 1)).  Writing image files is the caller's."""
    with torch.no_grad():
        rendered, _, _ = renderer_grid(cameras=camera, volumetric_function=field.batched_forward)
        last = rendered.shape[-1]
        return rendered[0].split([last - 1, 1], dim=-1)
