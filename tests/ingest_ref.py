"""NumPy restatement of include/isr_ingest.h (test infrastructure): the per-frame body of cowrendersynth.generate_bop_realsamples
as the header states it, written the way the reference writes it — the canvas IS materialised here, the box comes from
np.nonzero, the resize is vectorised over the output grid — so it shares no code path with csrc/ingest.hpp.  NumPy does not
contract a * b + c, so the f64 sums round as the library's do under -ffp-contract=off.

`mutate` names one deliberate departure from the rule (tests/test_ingest_cpu.py checks that each is caught):
    no_even_cut      an odd w2 / h2 keeps its last column / row
    swap_hw_hh       hs1 - hw and hs1 - hh change places in the canvas placement and the camera shift
    align_corners    sx = dx (side - 1) / (maxB - 1)
    zero_border      neighbours outside the canvas count as 0 instead of the edge pixel
    gate_ch0         mask channel 0 gates all three colours
    k_scale_first    K * (maxB / side) in place of (K * maxB) / side
Also here: the case list that the CPU and GPU tests share."""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64
MUTATIONS = ("no_even_cut", "swap_hw_hh", "align_corners", "zero_border", "gate_ch0", "k_scale_first")
NAN_BITS = 0x7ff8000000000000


def bounding_rect(m0):
    """cv2.boundingRect of a 2-D u8 array: (x, y, w, h) of the non-zero pixels, (0, 0, 0, 0) when there are none."""
    ys, xs = np.nonzero(m0)
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def geometry(box, offset, mutate=None):
    """(x2, y2, w2, h2, hw, hh, side, hs1) from the box before the even cut."""
    x2, y2, w2, h2 = box
    if mutate != "no_even_cut":
        if w2 % 2 != 0:
            w2 = w2 - 1
        if h2 % 2 != 0:
            h2 = h2 - 1
    hw, hh = int(w2 / 2), int(h2 / 2)
    maxd = int(max(w2, h2))
    side = maxd + 2 * offset
    return x2, y2, w2, h2, hw, hh, side, int(side / 2)


def gated(rgb, mask, mutate=None):
    """c1[np.where(m1 == 0)] = 0 with m1 of three channels (a one-channel mask read as three equal ones)."""
    m3 = np.repeat(mask, 3, axis=2) if mask.shape[2] == 1 else mask
    if mutate == "gate_ch0":
        m3 = np.repeat(mask[:, :, :1], 3, axis=2)
    c1 = rgb.copy()
    c1[np.where(m3 == 0)] = 0
    return c1


def canvases(rgb, mask, g, mutate=None):
    """squareRGB1 (side, side, 3) and squareMask1 (side, side) u8, as cowrendersynth.py:678-685 builds them."""
    x2, y2, w2, h2, hw, hh, side, hs1 = g
    c1 = gated(rgb, mask, mutate)
    sq = np.zeros((side, side, 3), np.uint8)
    sm = np.zeros((side, side), np.uint8)
    a, b = (hw, hh) if mutate == "swap_hw_hh" else (hh, hw)      # the rule: rows by hh, columns by hw
    ys, xs = slice(hs1 - a, hs1 - a + 2 * hh), slice(hs1 - b, hs1 - b + 2 * hw)
    if mutate == "no_even_cut":
        ys, xs = slice(hs1 - hh, hs1 - hh + h2), slice(hs1 - hw, hs1 - hw + w2)
    sq[ys, xs] = c1[y2:y2 + h2, x2:x2 + w2]
    sm[ys, xs] = mask[y2:y2 + h2, x2:x2 + w2, 0]
    return sq, sm


def _axis(side, maxB, mutate):
    d = np.arange(maxB, dtype=f64)
    if mutate == "align_corners":
        s = d * (side - 1) / max(maxB - 1, 1)
    else:
        s = ((d + 0.5) * side) / maxB - 0.5
    f0 = np.floor(s)
    return f0.astype(np.int64), s - f0


def bilinear_f64(img, maxB, mutate=None):
    """The f64 bilinear sum of a (side, side[, C]) u8 image at the maxB x maxB grid, before the rounding."""
    side = img.shape[0]
    a = img.astype(f64)
    if a.ndim == 2:
        a = a[:, :, None]
    i0, fr = _axis(side, maxB, mutate)
    i1 = i0 + 1

    def take(yi, xi):
        yc, xc = np.clip(yi, 0, side - 1), np.clip(xi, 0, side - 1)
        v = a[yc[:, None], xc[None, :]]
        if mutate == "zero_border":
            ok = ((yi >= 0) & (yi < side))[:, None] & ((xi >= 0) & (xi < side))[None, :]
            v = v * ok[:, :, None]
        return v

    fy, fx = fr[:, None, None], fr[None, :, None]
    w00, w01, w10, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
    v = ((take(i0, i0) * w00 + take(i0, i1) * w01) + take(i1, i0) * w10) + take(i1, i1) * w11
    return v if img.ndim == 3 else v[:, :, 0]


def resize_linear(img, maxB, mutate=None):
    return np.rint(bilinear_f64(img, maxB, mutate)).astype(np.uint8)


def resize_nearest(img, maxB):
    side = img.shape[0]
    i = (np.arange(maxB, dtype=np.int64) * side) // maxB
    return img[i[:, None], i[None, :]]


def camera(K, g, maxB, make_ndc, mutate=None):
    """cowrendersynth.py:717-736 -> KObj[a11] (4, 4)."""
    x2, y2, w2, h2, hw, hh, side, hs1 = g
    if side == 0:
        return np.full((4, 4), np.nan)
    cam = np.asarray(K, f64).reshape(3, 3).copy()
    a, b = (hh, hw) if mutate == "swap_hw_hh" else (hw, hh)
    cam[0, 2] = cam[0, 2] + (-x2 + hs1 - a)
    cam[1, 2] = cam[1, 2] + (-y2 + hs1 - b)
    cam = cam * (maxB / side) if mutate == "k_scale_first" else cam * maxB / side
    cam[2, 2] = 1
    if make_ndc:
        cam = cam * 2 / maxB
        cam[2, 2] = 0
        cam[0, 2] = -(cam[0, 2] - 1)
        cam[1, 2] = -(cam[1, 2] - 1)
    out = np.zeros((4, 4))
    out[0:3, 0:3] = cam
    out[3, 2] = 1
    out[2, 3] = 1
    return out


def ingest(rgb, mask, K, maxB, offset=10, make_ndc=True, silhouette="linear", mutate=None):
    """-> images (n, maxB, maxB, 3) f32, silhouettes (n, maxB, maxB) f32, K_out (n, 4, 4) f64, geom (n, 8) i32, status (n,) i32."""
    rgb, mask = np.asarray(rgb, np.uint8), np.asarray(mask, np.uint8)
    if mask.ndim == 3:
        mask = mask[..., None]
    n = rgb.shape[0]
    images, sil = np.zeros((n, maxB, maxB, 3), f32), np.zeros((n, maxB, maxB), f32)
    K_out, geom, status = np.zeros((n, 4, 4)), np.zeros((n, 8), np.int32), np.zeros(n, np.int32)
    for i in range(n):
        g = geometry(bounding_rect(mask[i, :, :, 0]), offset, mutate)
        geom[i] = g
        K_out[i] = camera(np.asarray(K, f64).reshape(n, 9)[i], g, maxB, make_ndc, mutate)
        if g[6] == 0:
            status[i] = 1
            continue
        sq, sm = canvases(rgb[i], mask[i], g, mutate)
        images[i] = resize_linear(sq, maxB, mutate).astype(f32) / f32(255)
        s8 = resize_nearest(sm, maxB) if silhouette == "nearest" else resize_linear(sm, maxB, mutate)
        sil[i] = s8.astype(f32) / f32(255)
    return images, sil, K_out, geom, status


def same(a, b) -> bool:
    """Bit equality of two arrays of one dtype and shape (NaN-aware, -0.0-aware)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the shared case list
SIZES = ((1, 1), (1, 7), (7, 1), (5, 8), (17, 33), (33, 17))      # (H, W)
BOX_KINDS = ("corner", "edges", "pixel", "odd_even", "wide", "tall", "empty")
OFFSETS = (0, 1, 5, 10)
MAX_BS = (1, 2, 7, 33)
N_FRAMES = 17


def box_for(kind, H, W):
    """(x, y, w, h) of a kind of box inside an H x W frame (clipped to it)."""
    x, y, w, h = {"corner": (0, 0, 3, 2), "edges": (0, 0, W, H), "pixel": (W // 2, H // 2, 1, 1), "odd_even": (1, 1, 5, 4),
                  "wide": (1, 2, 12, 3), "tall": (2, 1, 3, 12), "empty": (0, 0, 0, 0)}[kind]
    x, y = min(x, W - 1), min(y, H - 1)
    return x, y, min(w, W - x), min(h, H - y)


def frames(H, W, Cm, seed=0):
    """N_FRAMES frames of H x W: one per box kind (the box's corners set, its inside random), the rest random blobs.
    A three-channel mask's channels differ: channels 1 and 2 drop pixels of their own.  -> rgb, mask, K (n, 9), kinds."""
    rng = np.random.default_rng([seed, H, W, Cm])
    rgb = rng.integers(1, 256, (N_FRAMES, H, W, 3), dtype=np.uint8)      # no zero colours: a gate that fails shows
    mask = np.zeros((N_FRAMES, H, W, Cm), np.uint8)
    kinds = []
    for i in range(N_FRAMES):
        kind = BOX_KINDS[i] if i < len(BOX_KINDS) else "random"
        kinds.append(kind)
        if kind == "random":
            x, w = sorted(rng.integers(0, W + 1, 2))
            y, h = sorted(rng.integers(0, H + 1, 2))
            x, y, w, h = int(x), int(y), int(w - x), int(h - y)
        else:
            x, y, w, h = box_for(kind, H, W)
        if w == 0 or h == 0:
            continue
        inside = rng.choice(np.array([0, 1, 128, 255], np.uint8), (h, w, Cm), p=[0.3, 0.2, 0.2, 0.3])
        inside[0, 0, 0] = inside[-1, -1, 0] = inside[0, -1, 0] = inside[-1, 0, 0] = 255      # the box is exactly (x, y, w, h)
        mask[i, y:y + h, x:x + w] = inside
    K = np.tile(np.array([572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0]), (N_FRAMES, 1))
    K[:, 2] += rng.uniform(-3, 3, N_FRAMES)
    K[:, 5] += rng.uniform(-3, 3, N_FRAMES)
    return rgb, mask, K, kinds


def params():
    """Every (maxB, offset, make_ndc, silhouette) of the sweep."""
    for maxB in MAX_BS:
        for offset in OFFSETS:
            for ndc in (False, True):
                for sil in ("linear", "nearest"):
                    yield maxB, offset, ndc, sil


def batches(H, W, Cm):
    """The sweep of one frame shape: dicts of rgb, mask, K, max_b, offset, make_ndc, silhouette.  n = 17 under every
    parameter; n = 2 (the pixel box and the odd x even one: with offset 0 a side-0 frame beside an ordinary one) and n = 1
    (every kind in turn) under the parameters they can tell apart."""
    rgb, mask, K, kinds = frames(H, W, Cm)
    for j, (maxB, offset, ndc, sil) in enumerate(params()):
        kw = dict(max_b=maxB, offset=offset, make_ndc=ndc, silhouette=sil)
        yield dict(rgb=rgb, mask=mask, K=K, **kw)
        yield dict(rgb=rgb[2:4], mask=mask[2:4], K=K[2:4], **kw)
        i = j % N_FRAMES
        yield dict(rgb=rgb[i:i + 1], mask=mask[i:i + 1], K=K[i:i + 1], **kw)


# ---------------------------------------------------------------- a BOP folder on disk
def write_bop_tree(root, rgb, mask, K, R, T, objid="22", lmDir="train", diameter=142.5, ids=None, order="bgr"):
    """A BOP tree under `root` for frames rgb (n, H, W, 3) / mask (n, H, W, Cm) given in `order` (what read_bop_frames is to
    return under its default): <lmDir>/0000<objid>/{rgb,mask}/*.png, scene_camera.json, scene_gt.json, scene_gt_info.json and
    models/models_info.json.  Floats are written with repr: they read back bit for bit.  -> the object's folder."""
    import json
    from pathlib import Path

    from PIL import Image
    root = Path(root)
    obj = root / lmDir / ("0000" + str(objid).zfill(2))
    (obj / "rgb").mkdir(parents=True)
    (obj / "mask").mkdir()
    (root / "models").mkdir(exist_ok=True)
    n = rgb.shape[0]
    ids = list(range(n)) if ids is None else [int(i) for i in ids]
    cam, gt, info = {}, {}, {}
    for k, i in enumerate(ids):
        c, m = rgb[k], mask[k]
        if order == "bgr":
            c, m = c[..., ::-1], m[..., ::-1]
        Image.fromarray(np.ascontiguousarray(c), "RGB").save(obj / "rgb" / f"{i:06d}.png")
        (Image.fromarray(np.ascontiguousarray(m[..., 0]), "L") if m.shape[2] == 1 else Image.fromarray(np.ascontiguousarray(m), "RGB")).save(
            obj / "mask" / f"{i:06d}_000000.png")
        cam[str(i)] = {"cam_K": [float(v) for v in np.asarray(K[k]).reshape(9)], "depth_scale": 1.0}
        gt[str(i)] = [{"cam_R_m2c": [float(v) for v in np.asarray(R[k]).reshape(9)], "cam_t_m2c": [float(v) for v in T[k]], "obj_id": int(objid)}]
        info[str(i)] = [{"bbox_obj": [0, 0, 1, 1], "bbox_visib": [0, 0, 1, 1], "visib_fract": 1.0}]
    (obj / "scene_camera.json").write_text(json.dumps(cam))
    (obj / "scene_gt.json").write_text(json.dumps(gt))
    (obj / "scene_gt_info.json").write_text(json.dumps(info))
    (root / "models" / "models_info.json").write_text(json.dumps({str(objid): {"diameter": float(diameter)}}))
    return obj


def folder_frames(n=4, H=24, W=32, Cm=3, seed=7):
    """n frames of H x W with blob masks holding 0/255 (so "nearest" gives 0/1), cameras and poses -> rgb, mask, K (n, 3, 3), R, T."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(1, 256, (n, H, W, 3), dtype=np.uint8)
    mask = np.zeros((n, H, W, Cm), np.uint8)
    for i in range(n):
        x, y, w, h = 3 + i, 2 + i, 12 + 2 * i, 9 + i
        blob = rng.choice(np.array([0, 255], np.uint8), (h, w, 1), p=[0.2, 0.8])
        blob[0, 0] = blob[-1, -1] = 255
        mask[i, y:y + h, x:x + w] = blob
    K = np.tile(np.array([[572.4114, 0.0, 16.3], [0.0, 573.57043, 12.1], [0.0, 0.0, 1.0]]), (n, 1, 1))
    K[:, 0:2, 2] += rng.uniform(-2, 2, (n, 2))
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    T = np.stack([rng.uniform(-80, 80, n), rng.uniform(-80, 80, n), rng.uniform(500, 800, n)], 1)
    return rgb, mask, K, q, T
