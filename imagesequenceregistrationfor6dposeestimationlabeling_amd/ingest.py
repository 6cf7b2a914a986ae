"""Sequence ingest: a BOP folder to training views and cameras (SURVEY §1's layer L0).

Four of the reference's scripts begin with cowrendersynth.generate_bop_realsamples (cowrendersynth.py:610-747):
trainNerfFine.py:84-87, generateCors.py:97, trainPose.py:87 and genFeat.py:63.  This module is that call with the per-frame
cv2 loop replaced by ops.ingest_views (include/isr_ingest.h states the rule: the gate, the box, the square canvas with its
margin, the resize to maxB and the camera matrix that follows the box), and the block every script repeats after it:

    read_bop_frames            rgb/%06d.png and <mask>/%06d_000000.png through PIL -> host u8 arrays
    extract_rt                 nutil.extractRT (nutil.py:129-138) over formats.read_scene_gt's data
    generate_bop_realsamples   the drop-in: the reference's positional order and return tuples, CPU tensors and NumPy arrays
    training_views             the id ranges of trainNerfFine.py:71-80, the ingest, the pose conversion of :91-101 and the depth
                               bounds of :118-119 -> TrainingViews, the images kept on the device
    TrainingViews.cameras      trainPose.py:272-286 -> rays.PerspectiveCameras

The silhouette: "linear" (the default) is what the reference's cv2.resize call does — its interpolation flag sits in the dst
slot, so the default INTER_LINEAR runs (from memory, unpinned: cv2 is not available); "nearest" is what the call says, and
gives the 0/1 silhouette augment.PoseBatches needs.

Out of scope: the `background` branch (its target_backgrounds list is ragged; augment.py lists that branch as out of scope
too), the other nine loaders of cowrendersynth.py, COCO / T-LESS occluder files, JPEG, depth images, and cv2's own bytes (the
resize is an owned textbook definition; cv2's 8-bit resize is fixed-point and can differ by a grey level).
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from . import formats, ops

__all__ = ["read_bop_frames", "extract_rt", "generate_bop_realsamples", "TrainingViews", "training_views"]


def _png(path: Path):
    from PIL import Image
    if not path.exists():
        raise FileNotFoundError(f"ingest: {path} is missing")
    return Image.open(path)


def read_bop_frames(obj_dir, ids, mask_str: str = "mask", channel_order: str = "bgr"):
    """rgb/%06d.png and <mask_str>/%06d_000000.png of the frames `ids` -> (rgb (n, H, W, 3) u8, mask (n, H, W, Cm) u8) on the host.
    channel_order "bgr" (the default: cv2.imread gives it and the reference keeps it) or "rgb"; a three-channel mask follows
    it, so channel 0 is the one cv2 would call channel 0.  A grey mask stays one channel (cv2.imread would repeat it three
    times: the same gate).  Frames of different sizes raise ValueError."""
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"read_bop_frames: channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    obj_dir = Path(obj_dir)
    rgbs, masks = [], []
    for i in ids:
        name = str(int(i)).zfill(6)
        c = np.asarray(_png(obj_dir / "rgb" / f"{name}.png").convert("RGB"), np.uint8)
        m = _png(obj_dir / mask_str / f"{name}_000000.png")
        m = np.asarray(m.convert("L"), np.uint8)[..., None] if m.mode in ("1", "L", "I", "I;16", "F") else np.asarray(m.convert("RGB"), np.uint8)
        if channel_order == "bgr":
            c, m = c[..., ::-1], m[..., ::-1]
        if m.shape[:2] != c.shape[:2]:
            raise ValueError(f"read_bop_frames: frame {int(i)}: rgb is {c.shape[:2]} and its mask {m.shape[:2]}")
        if rgbs and (c.shape != rgbs[0].shape or m.shape != masks[0].shape):
            raise ValueError(f"read_bop_frames: frame {int(i)} is {c.shape[:2]} with {m.shape[2]} mask channel(s), "
                             f"the frames before it {rgbs[0].shape[:2]} with {masks[0].shape[2]}: sizes cannot be mixed")
        rgbs.append(c)
        masks.append(m)
    if not rgbs:
        raise ValueError("read_bop_frames: no ids")
    return np.ascontiguousarray(np.stack(rgbs)), np.ascontiguousarray(np.stack(masks))


def extract_rt(scene_gt, image_id, occid: int = 0):
    """nutil.extractRT: the pose of instance `occid` in frame `image_id` -> (R (3, 3), T (3,)) f64.  scene_gt: the path of a
    scene_gt.json, or what formats.read_scene_gt(path, obj_index=occid) returned."""
    if isinstance(scene_gt, (str, Path)):
        scene_gt = formats.read_scene_gt(scene_gt, obj_index=occid)
    ids, R, t = scene_gt
    try:
        k = list(ids).index(int(image_id))
    except ValueError:
        raise KeyError(f"extract_rt: frame {int(image_id)} is not in scene_gt") from None
    return R[k].copy(), t[k].copy()


def _object_dir(datasetPath, objid, dataset: str, synth: bool, lmDir: str) -> tuple[Path, Path]:
    """cowrendersynth.py:616-624 -> (the frames' folder, the folder of scene_gt_info.json)."""
    if dataset == "lm":
        lmDir = "lm_synth" if synth else "lm"
    base = Path(str(datasetPath)) / lmDir
    return base / ("0000" + str(objid).zfill(2)), base / str(objid).zfill(6)


def _ingest_ids(obj_dir: Path, ids, K_all, mask_str, channel_order, max_b, offset, make_ndc, silhouette, device, chunk, keep_on_device):
    """The frames `ids` through ops.ingest_views in chunks -> images, silhouettes (device tensors, or CPU ones), K (n, 4, 4) f64."""
    if int(chunk) < 1:
        raise ValueError(f"ingest: chunk = {chunk}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    images, sils, Ks, stats = [], [], [], []
    shape = None
    for c0 in range(0, len(ids), int(chunk)):
        part = ids[c0:c0 + int(chunk)]
        rgb, mask = read_bop_frames(obj_dir, part, mask_str, channel_order)
        if shape is not None and (rgb.shape[1:], mask.shape[1:]) != shape:
            raise ValueError(f"ingest: frames {int(part[0])}.. are {rgb.shape[1:3]}, the frames before them {shape[0][:2]}: sizes cannot be mixed")
        shape = (rgb.shape[1:], mask.shape[1:])
        K = np.ascontiguousarray(K_all[c0:c0 + int(chunk)], np.float64)
        if dev.type == "cpu":
            v = ops.ingest_views_host(rgb, mask, K, max_b, offset, make_ndc, silhouette)
            v = ops.IngestedViews(*(torch.from_numpy(a) for a in v))
        else:
            v = ops.ingest_views(torch.from_numpy(rgb).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(K).to(dev), max_b,
                                 offset, make_ndc, silhouette)
        images.append(v.images if keep_on_device else v.images.cpu())
        sils.append(v.silhouettes if keep_on_device else v.silhouettes.cpu())
        Ks.append(v.K)
        stats.append(v.status)
    status = torch.cat(stats).cpu().numpy()                     # the one host read of status
    bad = np.nonzero(status)[0]
    if bad.size:
        raise ValueError(f"ingest: frame {int(ids[int(bad[0])])} has a mask box of at most one pixel a side and offset 0: "
                         f"its square has side 0 ({bad.size} such frame(s))")
    return torch.cat(images), torch.cat(sils), torch.cat(Ks).cpu().numpy()


def _poses_and_cameras(obj_dir: Path, ids):
    cam_ids, K = formats.read_scene_camera(obj_dir / "scene_camera.json")
    gt_ids, R, t = formats.read_scene_gt(obj_dir / "scene_gt.json", obj_index=0)
    cam_at, gt_at = {v: k for k, v in enumerate(cam_ids)}, {v: k for k, v in enumerate(gt_ids)}
    for i in ids:
        if int(i) not in cam_at or int(i) not in gt_at:
            raise KeyError(f"ingest: frame {int(i)} is not in scene_camera.json / scene_gt.json of {obj_dir}")
    rows = [int(i) for i in ids]
    return (np.stack([K[cam_at[i]] for i in rows]), np.stack([R[gt_at[i]] for i in rows]), np.stack([t[gt_at[i]] for i in rows]),
            len(cam_ids))


def _frame_count(obj_dir: Path, info_dir: Path) -> tuple[int, int]:
    n_cam = len(json.loads((obj_dir / "scene_camera.json").read_text()))
    n_info = len(json.loads((info_dir / "scene_gt_info.json").read_text()))
    return n_cam, n_info


def generate_bop_realsamples(datasetPath, objid="22", imD=128, crop=True, maskStr="mask", cropDim=70, justScaleImages=False,
                             ScaledSize=128, maxB=200, offset=10, synth=True, makeNDC=True, dataset="tless", fewSamps=False,
                             fewCT=20, fewids=[0], background=False, lmDir="train", *, device=None, chunk=64, seed=0,
                             silhouette="linear", channel_order="bgr"):
    """cowrendersynth.generate_bop_realsamples, the drop-in: the reference's positional order, and its return tuples
        (target_images (n, maxB, maxB, 3), target_silhouettes (n, maxB, maxB), RObj (n, 3, 3), TObj (n, 3), KObj (n, 4, 4))
    with `lines` appended when fewSamps — CPU f32 tensors and f64 NumPy arrays, as the reference returns them.  imD, crop,
    cropDim, justScaleImages and ScaledSize are accepted and not read, as in the reference.
    The frames go through the device (`device`, default the current one; "cpu": the library's host build) `chunk` at a time;
    status is read once, at the end, and a frame whose square has side 0 raises ValueError.
    fewSamps with len(fewids) == 1 draws fewCT ids from np.random.default_rng(seed) — an owned rule: the reference's
    np.random.random_integers is unseeded and gone from current NumPy.  background=True raises NotImplementedError."""
    if background:
        raise NotImplementedError("generate_bop_realsamples: background=True (the ragged target_backgrounds list) is out of scope")
    obj_dir, info_dir = _object_dir(datasetPath, objid, dataset, synth, lmDir)
    imCT, n_info = _frame_count(obj_dir, info_dir)
    lines = None
    if not fewSamps:
        if n_info < imCT:
            raise ValueError(f"generate_bop_realsamples: scene_gt_info.json lists {n_info} frames, scene_camera.json {imCT}")
        ids = np.arange(imCT)
    else:
        if len(fewids) == 1:
            fewids = np.random.default_rng(seed).integers(0, imCT, int(fewCT))
            lines = np.arange(imCT)[fewids]
        else:
            lines = fewids
        ids = np.asarray([int(v) for v in lines], np.int64)
    K_in, R, T, _ = _poses_and_cameras(obj_dir, ids)
    images, sils, KObj = _ingest_ids(obj_dir, ids, K_in, maskStr, channel_order, int(maxB), int(offset), bool(makeNDC), silhouette,
                                     device, chunk, keep_on_device=False)
    if fewSamps:
        return images, sils, R, T, KObj, lines
    return images, sils, R, T, KObj


def rot_from_euler(x: float, y: float, z: float) -> np.ndarray:
    """Rz(z) Ry(y) Rx(x) in f64, the product taken as Rz . (Ry . Rx): nutil.rotfromeulernp's arithmetic."""
    cx, sx, cy, sy, cz, sz = np.cos(x), np.sin(x), np.cos(y), np.sin(y), np.cos(z), np.sin(z)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return np.dot(rz, np.dot(ry, rx))


def convert_poses(R, T, diameter: float, diam_scaling: float = 1.8):
    """trainNerfFine.py:91-101: R[a] = R[a]^T rot180, T[a, 0:2] = -T[a, 0:2], T = T / (diameter / diam_scaling), with rot180 =
    rot_from_euler(0, 0, pi) — sin(pi)'s 1.2e-16 included, as the scripts have it.  -> new (R, T)."""
    R, T = np.array(R, np.float64), np.array(T, np.float64)
    rot180 = rot_from_euler(0.0, 0.0, np.pi)
    for a in range(R.shape[0]):
        R[a] = (R[a].T).dot(rot180)
        T[a, 0:2] = -T[a, 0:2]
    return R, T / (diameter / diam_scaling)


@dataclass
class TrainingViews:
    """What the scripts hold after their first block: images (n, B, B, 3) and silhouettes (n, B, B) f32 on the device; R (n, 3, 3),
    T (n, 3) (converted, in object diameters / 1.8) and K (n, 4, 4) f64 on the host; ids; the two depth bounds."""
    images: torch.Tensor
    silhouettes: torch.Tensor
    R: np.ndarray
    T: np.ndarray
    K: np.ndarray
    ids: np.ndarray
    min_depth: float
    volume_extent_world: float

    def __len__(self) -> int:
        return int(self.images.shape[0])

    def cameras(self, idx, imD: int, in_ndc: bool):
        """trainPose.py:272-286: the cameras of the views `idx` -> rays.PerspectiveCameras on the images' device: focal length
        (K[0][0], K[1][1]), principal point (K[0][2], K[1][2]), image size imD x imD."""
        from .rays import PerspectiveCameras
        idx = np.atleast_1d(np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, np.int64))
        K = self.K[idx].astype(np.float32)
        focal = K[:, 0, 0:2].copy()
        focal[:, 1] = K[:, 1, 1]
        principal = K[:, 0:2, 2].copy()
        return PerspectiveCameras(R=torch.from_numpy(self.R[idx].astype(np.float32)), T=torch.from_numpy(self.T[idx].astype(np.float32)),
                                  focal_length=torch.from_numpy(focal), principal_point=torch.from_numpy(principal),
                                  image_size=(int(imD), int(imD)), in_ndc=bool(in_ndc), device=self.images.device)


def training_ids(dataset: str, UH) -> np.ndarray:
    """trainNerfFine.py:71-80: the lower half of the sequence when UH, else the upper one (T-LESS: 500 of 1 000 frames)."""
    if dataset == "tless":
        ids = np.arange(int(1001 * 0.5))
        return ids if int(UH) else ids + 500
    ids = np.arange(int(2561 * 0.5))
    return ids if int(UH) else ids + 1280


def training_views(datasetPath, objid, dataset: str, UH, *, max_b: int, device, diameter: float | None = None, offset: int = 5,
                   mask_str: str = "mask", make_ndc: bool = False, silhouette: str = "linear", chunk: int = 64, ids=None,
                   synth: bool = False, lmDir: str = "train", channel_order: str = "bgr") -> TrainingViews:
    """The block every script repeats (trainNerfFine.py:71-119): the id range of (dataset, UH) (or `ids`), the ingest with the
    scripts' arguments (offset 5, synth False, makeNDC = in_ndc = False), the pose conversion and the two depth bounds
    min |T_z| - 2 and max |T_z| + 2.  diameter: the object's, default models/models_info.json's entry for objid.
    The images stay on `device`."""
    obj_dir, _ = _object_dir(datasetPath, objid, dataset, synth, lmDir)
    ids = training_ids(dataset, UH) if ids is None else np.asarray([int(v) for v in ids], np.int64)
    K_in, R, T, _ = _poses_and_cameras(obj_dir, ids)
    images, sils, K = _ingest_ids(obj_dir, ids, K_in, mask_str, channel_order, int(max_b), int(offset), bool(make_ndc), silhouette,
                                  device, chunk, keep_on_device=True)
    if diameter is None:
        info = json.loads((Path(str(datasetPath)) / "models" / "models_info.json").read_text())
        diameter = info[str(objid)]["diameter"]
    R, T = convert_poses(R, T, diameter)
    min_depth = np.min(np.abs(T[:, 2])) - 2
    volume_extent_world = np.max(np.abs(T[:, 2])) + 2
    return TrainingViews(images, sils, R, T, K, ids, float(min_depth), float(volume_extent_world))
