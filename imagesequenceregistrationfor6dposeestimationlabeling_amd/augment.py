"""Training batches on the device: from device-resident training views and their correspondences to the arguments of
training.pose_train_step, with no host round trip per batch.  What dataGen.AugmentedSamples gets from
augment.generateImages (augment.py:284-432), dataGen.normalize (dataGen.py:16-20) and augment.getNerfSamples
(augment.py:639-685), through ops.augment_images and ops.augment_rays (include/isr_augment.h states their rules).

The host's part is the parameter draw (draw_params: a few numbers per image from a seeded CPU generator, augment.py:315-342);
every output is a function of the inputs and the seed.

The albumentations colour pass (augment.py:344-350, applied at :394-397 and :422-423) is ops.augment_color under programs
drawn by draw_color_params, as owned definitions (include/isr_color_aug.h states them and what differs from the libraries):
PoseBatches(color=True) opts in.

Out of scope: albumentations' and cv2's own bytes and draws (LAB-space CLAHE, cv2's 8-bit HSV, blur sizes above 3, image sides
that are no multiple of 8); reading COCO / T-LESS files and the T-LESS occluder paste (`canvases` is
what rgbtensor[a] already holds); the target_backgrounds branch; lineErode; the NOCS map (trainPose.py computes it, its loss
does not read it); and the 0/255 mask branch, where the reference's `== 1` never matches.  cv2.getRotationMatrix2D's formula is
the documented one, from memory: unpinned."""
from __future__ import annotations

import math
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from . import formats, ops

__all__ = ["AugmentParams", "ColorParams", "CorrespondenceBank", "PoseBatches", "draw_color_params", "draw_params", "ray_transform",
           "rotation_matrix_2d"]


def rotation_matrix_2d(center, angle_deg, scale) -> np.ndarray:
    """cv2.getRotationMatrix2D(center, angle, scale) as OpenCV documents it, in f64 -> (2, 3):
        a = scale cos(angle), b = scale sin(angle);   [[a, b, (1 - a) cx - b cy], [-b, a, b cx + (1 - a) cy]]
    with the angle in degrees, positive counter-clockwise (the origin at the top left)."""
    ang = float(angle_deg) * math.pi / 180.0
    a, b = float(scale) * math.cos(ang), float(scale) * math.sin(ang)
    cx, cy = float(center[0]), float(center[1])
    return np.array([[a, b, (1.0 - a) * cx - b * cy], [-b, a, b * cx + (1.0 - a) * cy]], np.float64)


def ray_transform(rot_deg, scale, tra, imD) -> tuple[np.ndarray, np.ndarray]:
    """What augment.py:647-648 applies to a view's ray locations, for B images: rot (B, 4) f32 = (m00, m01, m10, m11) of
    getRotationMatrix2D((0, 0), trR, float(trS)) cast to f32 — trS has been through dataGen's f32 tensor — and t (B, 2) f32 =
    trT / (imD / 2), an f32 division."""
    rot_deg, scale = np.asarray(rot_deg).reshape(-1), np.asarray(scale, np.float64).reshape(-1)
    rot = np.stack([rotation_matrix_2d((0, 0), int(r), float(np.float32(s)))[:, :2].astype(np.float32).reshape(4)
                    for r, s in zip(rot_deg, scale)])
    t = np.asarray(tra, np.float32).reshape(-1, 2) / np.float32(float(imD) / 2)
    return rot, t.astype(np.float32)


@dataclass
class AugmentParams:
    """The per-image parameters of one batch, plain CPU tensors (build one by hand for a fixed augmentation):
    M (B, 2, 3) f64 source -> destination; tra, tra1 (B, 2) i32; rect (B, 4) i32 = (x, y, w, h), w = 0 or h = 0: none;
    border (B, 2) i32 = (kh, kw), 0 = off; rot_deg (B,) i32 and scale (B,) f64 (trR, trS); ray_rot (B, 4) and ray_t (B, 2) f32
    (ray_transform)."""
    M: torch.Tensor
    tra: torch.Tensor
    tra1: torch.Tensor
    rect: torch.Tensor
    border: torch.Tensor
    rot_deg: torch.Tensor
    scale: torch.Tensor
    ray_rot: torch.Tensor
    ray_t: torch.Tensor

    def __len__(self) -> int:
        return int(self.M.shape[0])


def mask_integral(masks: torch.Tensor) -> np.ndarray:
    """Summed-area tables of masks (B, H, W) -> (B, H + 1, W + 1) int64 on the host (torch's cumsum): what draw_params needs for
    the occluder's `sum > maskMax` acceptance."""
    m = masks.to(torch.int64)
    s = torch.zeros((m.shape[0], m.shape[1] + 1, m.shape[2] + 1), dtype=torch.int64, device=m.device)
    s[:, 1:, 1:] = m.cumsum(1).cumsum(2)
    return s.cpu().numpy()


def _rect_sum(integral: np.ndarray, x: int, y: int, w: int, h: int) -> int:
    H, W = integral.shape[0] - 1, integral.shape[1] - 1
    x0, y0, x1, y1 = min(max(x, 0), W), min(max(y, 0), H), min(max(x + w, 0), W), min(max(y + h, 0), H)
    return int(integral[y1, x1] - integral[y0, x1] - integral[y1, x0] + integral[y0, x0])


def draw_params(B: int, seed, H: int, *, bbox=None, integral=None, imD=None, scaleFac: float = 0.5, maxScale: float = 1.0,
                transScale: float = 1.0, transScale2: float = 0.2, surfEmbScaling: bool = False, surfEmbScaleFac: float = 1,
                maskErosion: bool = True, maskMax: float = 7000, borderADD: bool = False) -> AugmentParams:
    """The draws of augment.py:315-342 (and :425-426) for B square images of side H, from np.random.default_rng(seed); the
    reference's global NumPy stream is not reproduced.  Per image, in this order: the occluder (maskErosion and u > 0.3;
    createOcclusionsWithoutErosion's 0.3 / 0.99 cases; kept when the occluded mask's sum exceeds maskMax), randScale (the
    surfEmbScaling branch with its literal 224), randTra1, randTra (truncated toward zero), randRot = int(u * 360), the border
    kernel (borderADD and u > 0.6).  bbox (B, 4) = (x, y, w, h) from ops.mask_bbox (the un-occluded mask's: the occluder and
    surfEmbScaling need it), integral (B, H + 1, W + 1) from mask_integral (the occluder needs it).  imD: the divisor of the
    rays' translation, H when None."""
    rng = np.random.default_rng(seed)
    B, H = int(B), int(H)
    if bbox is not None:
        bbox = np.asarray(bbox.cpu() if isinstance(bbox, torch.Tensor) else bbox, np.int64).reshape(B, 4)
    if (maskErosion or surfEmbScaling) and bbox is None:
        raise ValueError("draw_params: maskErosion and surfEmbScaling need bbox")
    if maskErosion and integral is None:
        raise ValueError("draw_params: maskErosion needs integral (mask_integral of the batch's masks)")
    M = np.zeros((B, 2, 3), np.float64)
    tra, tra1 = np.zeros((B, 2), np.int64), np.zeros((B, 2), np.int64)
    rect, border = np.zeros((B, 4), np.int64), np.zeros((B, 2), np.int64)
    rot, scale = np.zeros(B, np.int64), np.zeros(B, np.float64)
    for b in range(B):
        if maskErosion and rng.uniform(0, 1) > 0.3:                                   # augment.py:315-318
            val = rng.uniform(0, 1)
            x, y, w, h = (int(v) for v in bbox[b])
            if val >= 0.3 and w > 0 and h > 0:                                        # :469-488
                nx, ny = int(rng.integers(x, x + w)), int(rng.integers(y, y + h))
                if val < 0.99:
                    r1, r2 = int(rng.integers(30, 70)), int(rng.integers(30, 70))
                else:
                    r1 = r2 = 30
                nw, nh = int(rng.integers(0, min(w, r1))), int(rng.integers(0, min(h, r2)))
                total = _rect_sum(integral[b], 0, 0, integral.shape[2], integral.shape[1])
                if total - _rect_sum(integral[b], nx, ny, nw, nh) > maskMax:
                    rect[b] = (nx, ny, nw, nh)
        s = (scaleFac + (1 - scaleFac) * rng.uniform(0, 1)) * maxScale                 # :331
        if surfEmbScaling:                                                            # :332-336
            w3, h3 = int(bbox[b, 2]), int(bbox[b, 3])
            s = 224 / max(w3, h3, 1) / 1.2 * rng.uniform(1 - 0.05 * surfEmbScaleFac, 1 + 0.05 * surfEmbScaleFac)
        tra1[b] = ((rng.uniform(0, 1, 2) - 0.5) * transScale2 * H / 2).astype("int64")      # :338
        tra[b] = ((rng.uniform(0, 1, 2) - 0.5) * transScale * H / 2).astype("int64")        # :340
        rot[b] = int(rng.uniform(0, 1) * 360)                                         # :342
        scale[b] = s
        M[b] = rotation_matrix_2d(((H - 1) / 2.0, (H - 1) / 2.0), rot[b], s)          # :354
        if borderADD and rng.uniform(0, 1) > 0.6:                                     # :425-426
            border[b] = (int(rng.integers(1, 20)), int(rng.integers(1, 20)))
    ray_rot, ray_t = ray_transform(rot, scale, tra, H if imD is None else imD)
    i32 = lambda a: torch.from_numpy(a.astype(np.int32))
    return AugmentParams(M=torch.from_numpy(M), tra=i32(tra), tra1=i32(tra1), rect=i32(rect), border=i32(border), rot_deg=i32(rot),
                         scale=torch.from_numpy(scale), ray_rot=torch.from_numpy(ray_rot), ray_t=torch.from_numpy(ray_t))


@dataclass
class ColorParams:
    """The colour programs of one pass over B images, plain CPU tensors (build one by hand for a fixed augmentation;
    ColorParams.neutral(B) has every gate off): include/isr_color_aug.h's isr_color_program, field for field.  apply, jitter,
    rbc, iso, clahe (B,) i32 gates (apply is the program's `pass`); order (B, 4) i32, a permutation of 0 brightness, 1 contrast,
    2 saturation, 3 hue; ksize (B,) i32: 0 off, else 1 or 3; the factors (B,) f64; noise_key (B,) i64."""
    apply: torch.Tensor
    jitter: torch.Tensor
    order: torch.Tensor
    rbc: torch.Tensor
    ksize: torch.Tensor
    iso: torch.Tensor
    clahe: torch.Tensor
    brightness: torch.Tensor
    contrast: torch.Tensor
    saturation: torch.Tensor
    hue: torch.Tensor
    alpha: torch.Tensor
    beta: torch.Tensor
    color_shift: torch.Tensor
    intensity: torch.Tensor
    clip_limit: torch.Tensor
    noise_key: torch.Tensor

    def __len__(self) -> int:
        return int(self.apply.shape[0])

    @classmethod
    def from_programs(cls, programs: np.ndarray) -> "ColorParams":
        f = lambda name, dt: torch.from_numpy(np.ascontiguousarray(programs[name]).astype(dt))
        return cls(apply=f("pass", np.int32), noise_key=f("noise_key", np.int64),
                   **{k: f(k, np.int32) for k in ("jitter", "order", "rbc", "ksize", "iso", "clahe")},
                   **{k: f(k, np.float64) for k in ("brightness", "contrast", "saturation", "hue", "alpha", "beta", "color_shift",
                                                    "intensity", "clip_limit")})

    @classmethod
    def neutral(cls, B: int) -> "ColorParams":
        return cls.from_programs(ops.color_programs(B))

    def programs(self) -> np.ndarray:
        """(B,) of ops.COLOR_PROGRAM: what ops.augment_color takes."""
        p = np.zeros(len(self), ops.COLOR_PROGRAM)
        for name in ops.COLOR_PROGRAM.names:
            t = getattr(self, "apply" if name == "pass" else name)
            p[name] = t.numpy().astype(np.uint64) if name == "noise_key" else t.numpy()
        return p


def draw_color_params(B: int, seed, *, p_pass: float = 0.7, p_jitter: float = 0.5, p_rbc: float = 0.2, p_blur: float = 0.5,
                      p_iso: float = 0.5, p_clahe: float = 0.5) -> ColorParams:
    """The draws of one albumentations pass (augment.py:344-350 under :394 / :422's `uniform > 0.3`) for B images, from
    np.random.default_rng(seed): a stream of its own, neither draw_params' nor albumentations'.  A gate is on when its
    uniform is below its probability.  Per image, in this order, every value drawn whether its gate is on or not: the pass
    gate; ColorJitter's gate, order (a permutation), brightness, contrast, saturation from U[0.8, 1.2], hue from U[-0.2, 0.2];
    RandomBrightnessContrast's gate, alpha = 1 + U(-0.2, 0.2), beta = U(-0.2, 0.2); GaussianBlur's gate and ksize from {1, 3};
    ISONoise's gate, color_shift from U[0.01, 0.05], intensity from U[0.1, 0.5], the noise key; CLAHE's gate and clip_limit
    from U[1, 4]."""
    rng = np.random.default_rng(seed)
    p = ops.color_programs(int(B))
    on = lambda prob: int(rng.uniform(0, 1) < prob)
    for b in range(int(B)):
        q = p[b]
        q["pass"] = on(p_pass)
        q["jitter"], q["order"] = on(p_jitter), rng.permutation(4)
        q["brightness"], q["contrast"], q["saturation"] = rng.uniform(0.8, 1.2, 3)
        q["hue"] = rng.uniform(-0.2, 0.2)
        q["rbc"], q["alpha"], q["beta"] = on(p_rbc), 1.0 + rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)
        blur, ksize = on(p_blur), int(rng.choice((1, 3)))
        q["ksize"] = ksize if blur else 0
        q["iso"], q["color_shift"], q["intensity"] = on(p_iso), rng.uniform(0.01, 0.05), rng.uniform(0.1, 0.5)
        q["noise_key"] = int(rng.integers(0, 2 ** 63))
        q["clahe"], q["clip_limit"] = on(p_clahe), rng.uniform(1.0, 4.0)
    return ColorParams.from_programs(p)


class CorrespondenceBank:
    """The correspondences of V views, concatenated on the device: per set (front, back) xys (sum n, 2) and pos (sum n, 3)
    f32, and the host offsets (V + 1) int64 — the layout of include/isr_augment.h."""

    def __init__(self, xys, pos, offsets, xys_back, pos_back, offsets_back):
        self.xys, self.pos, self.offsets = xys, pos, np.ascontiguousarray(offsets, np.int64)
        self.xys_back, self.pos_back, self.offsets_back = xys_back, pos_back, np.ascontiguousarray(offsets_back, np.int64)

    @classmethod
    def from_views(cls, views, device) -> "CorrespondenceBank":
        """views: one dict per view as formats.load_view_correspondences returns it (xys (1, n1, 2), pos_vec (1, n1, 3),
        pos_vec_back (1, n2, 3), xys_back (1, n2, 2)); a ViewCorrespondences works too."""
        views = list(views)
        if not views:
            raise ValueError("CorrespondenceBank: no views")
        get = lambda v, name: torch.as_tensor(v[name] if isinstance(v, dict) else getattr(v, name)).detach().to(torch.float32)
        out = []
        for xy_name, pos_name in (("xys", "pos_vec"), ("xys_back", "pos_vec_back")):
            xy = [get(v, xy_name).reshape(-1, 2) for v in views]
            ps = [get(v, pos_name).reshape(-1, 3) for v in views]
            for i, (a, p) in enumerate(zip(xy, ps)):
                if a.shape[0] != p.shape[0]:
                    raise ValueError(f"CorrespondenceBank: view {i} has {a.shape[0]} {xy_name} and {p.shape[0]} {pos_name}")
                if a.shape[0] > ops.AUGMENT_MAX_VIEW_ROWS:
                    raise ValueError(f"CorrespondenceBank: view {i} has more than 2^20 rows")
            off = np.concatenate([[0], np.cumsum([a.shape[0] for a in xy])]).astype(np.int64)
            out += [torch.cat(xy).to(device).contiguous(), torch.cat(ps).to(device).contiguous(), off]
        return cls(*out)

    @classmethod
    def from_dir(cls, nerf_dir: Path | str, render_size: int, views, device) -> "CorrespondenceBank":
        """The files generateCors.py writes (formats.save_view_correspondences), for the given view names."""
        return cls.from_views([formats.load_view_correspondences(nerf_dir, render_size, v) for v in views], device)

    def __len__(self) -> int:
        return int(self.offsets.size - 1)

    @property
    def front(self):
        return self.xys, self.pos, self.offsets

    @property
    def back(self):
        return self.xys_back, self.pos_back, self.offsets_back


class PoseBatches:
    """Iterating yields (rgb (B, H, W, 3), mask (B, H, W), pos_points (B, S, 3), xys (B, S, 2), extras), all on the device:
    the first four are training.pose_train_step's arguments — mask is the un-occluded mask_orig_out, the one trainPose.py:430's
    BCE reads (train_data[1]).  extras: mask_out, pos_points_back, xys_back, index, index_back, count, count_back (B,) i32,
    short (a 0-d bool on the device: some count, front or back, is below S — such rows are zeros with index -1, never padded),
    view_ids and params.

    images (V, H, H, 3) f32 and silhouettes (V, H, H) holding 0/1 on the device, bank: a CorrespondenceBank of the same V views.
    canvases (C, H, H, 3) f32 on the device or None: what generateImages' rgbtensor[a] holds before the paste; an image gets one
    with probability 0.9 (augment.py:300), else zeros.  Every iteration starts again from (seed, epoch): two fresh iterations
    give the same bytes; set_epoch changes the stream.  Batches are shuffled view indices, the last short one dropped.
    Between batches the host only draws parameters; nothing synchronises.

    color=True adds the albumentations pass, as generateImages applies it: a batch is made by ops.augment_images without
    canvas, border and normalize (mean 0 and std 1: exact identities in f32), then ops.augment_color over the warped object
    with select = mask_out and under = the canvas (:394-397 with the paste), then ops.augment_color over the composite with
    the border blanking and normalize as its tail (:422-428).  color_options: draw_color_params' keywords; the two passes'
    programs come from a generator of their own, [seed, epoch, k + 1, 1], and are extras["color_params"] = (first, second).
    The default route's bytes do not change, and p_pass = 0 gives them again.  H must then be a multiple of 8."""

    def __init__(self, images, silhouettes, bank: CorrespondenceBank, batch_size: int = 16, sample_size: int = 1024, seed: int = 0,
                 canvases=None, imD=None, mean=ops.IMAGENET_MEAN, std=ops.IMAGENET_STD, color: bool = False, color_options=None,
                 **draw_options):
        V = int(images.shape[0])
        if images.ndim != 4 or images.shape[3] != 3 or images.shape[1] != images.shape[2] or tuple(silhouettes.shape) != tuple(images.shape[:3]):
            raise ValueError(f"PoseBatches: images (V, H, H, 3) and silhouettes (V, H, H), got {tuple(images.shape)} and {tuple(silhouettes.shape)}")
        if len(bank) != V:
            raise ValueError(f"PoseBatches: {V} images and a bank of {len(bank)} views")
        if not 1 <= int(batch_size) <= V:
            raise ValueError(f"PoseBatches: batch_size {batch_size} for {V} views")
        if color and (int(images.shape[1]) % 8 or int(images.shape[1]) < 8):
            raise ValueError(f"PoseBatches: color=True needs an image side that is a multiple of 8, got {int(images.shape[1])}")
        self.color, self.color_options = bool(color), dict(color_options or {})
        self.images = images.to(torch.float32).contiguous()
        sil = silhouettes.to(torch.uint8)                                             # augment.py:286
        if int(sil.max()) >= 2:
            raise ValueError("PoseBatches: silhouettes must hold 0/1 (the 0/255 branch is out of scope)")
        self.masks = sil.contiguous()
        self.bank, self.batch_size, self.sample_size, self.seed, self.epoch = bank, int(batch_size), int(sample_size), int(seed), 0
        # one zero canvas appended: index C means "no canvas"
        self.canvases = None if canvases is None else torch.cat([canvases.to(torch.float32), torch.zeros_like(canvases[:1], dtype=torch.float32)])
        self.imD, self.mean, self.std, self.draw_options = imD, mean, std, draw_options
        self.bbox = ops.mask_bbox(self.masks).cpu().numpy()                           # once: the views do not change
        self.integral = mask_integral(self.masks) if draw_options.get("maskErosion", True) else None

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return int(self.images.shape[0]) // self.batch_size

    def __iter__(self):
        V, B, S, dev = int(self.images.shape[0]), self.batch_size, self.sample_size, self.images.device
        order = np.random.default_rng([self.seed, self.epoch]).permutation(V)
        for k in range(len(self)):
            ids = order[k * B:(k + 1) * B]
            rng = np.random.default_rng([self.seed, self.epoch, k + 1])
            draw_seed, ray_seed = (int(v) for v in rng.integers(0, 2 ** 63, 2))
            params = draw_params(B, draw_seed, int(self.images.shape[1]), bbox=self.bbox[ids], imD=self.imD,
                                 integral=None if self.integral is None else self.integral[ids], **self.draw_options)
            ids_dev = torch.from_numpy(ids.astype(np.int64)).to(dev)
            canvas = None
            if self.canvases is not None:
                C = int(self.canvases.shape[0]) - 1
                pick = torch.from_numpy(np.where(rng.uniform(0, 1, B) > 0.1, rng.integers(0, C, B), C)).to(dev)
                canvas = self.canvases[pick]
            masks = self.masks[ids_dev]
            geometry = dict(orig_mask=masks, rect=params.rect.numpy(), tra=params.tra.numpy(), tra1=params.tra1.numpy())
            color_params = None
            if self.color:
                seeds = np.random.default_rng([self.seed, self.epoch, k + 1, 1]).integers(0, 2 ** 63, 2)
                color_params = tuple(draw_color_params(B, int(s), **self.color_options) for s in seeds)
                warped, mask_orig, mask_out = ops.augment_images(self.images[ids_dev], masks, params.M.numpy(), canvas=None, border=None,
                                                                 mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), **geometry)
                pasted = ops.augment_color(warped, color_params[0].programs(), select=mask_out, under=canvas)
                rgb = ops.augment_color(pasted, color_params[1].programs(), border=params.border.numpy(), border_mask=mask_out,
                                        mean=self.mean, std=self.std)
            else:
                rgb, mask_orig, mask_out = ops.augment_images(self.images[ids_dev], masks, params.M.numpy(), canvas=canvas,
                                                              border=params.border.numpy(), mean=self.mean, std=self.std, **geometry)
            front, back = ops.augment_rays(self.bank.front, ids, params.ray_rot.numpy(), params.ray_t.numpy(), S, ray_seed,
                                           back=self.bank.back)
            extras = {"mask_out": mask_out, "pos_points_back": back.pos, "xys_back": back.xys, "index": front.index,
                      "index_back": back.index, "count": front.count, "count_back": back.count,
                      "short": ((front.count < S) | (back.count < S)).any(), "view_ids": ids_dev, "params": params, "color_params": color_params}
            yield rgb, mask_orig, front.pos, front.xys, extras
