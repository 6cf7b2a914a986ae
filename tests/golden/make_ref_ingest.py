#!/usr/bin/env python3
"""Generates ref_ingest.npz: the fixture that pins the geometry and the camera of isr_ingest_views, and the pose conversion of
ingest.training_views, to the reference's EXECUTED code.

  generate_bop_realsamples   cowrendersynth.py:667 (the gate), :669-690 (the even cut, the canvas, the centre) and :717-736 (KObj)
  the scripts' first block   trainNerfFine.py:91-101 (the pose conversion) and :118-119 (the depth bounds), with
                             nutil.rotfromeulernp executed for rot180

As the other make_ref_*.py do: nothing of the reference is imported or stored, the statements are parsed with `ast`, compiled
and executed, and only DATA is written.

What the statements are given that is not the reference's.  `cv2` is not available: the cv2.boundingRect line (:668) and the
two cv2.resize lines (:701-704) are left out, and the box is supplied as numbers — boxes chosen so that the mask's non-zero
pixels have exactly that box.  nutil.rotfromeulernp imports open3d and does not use it: an empty module of that name is put in
sys.modules while it runs.  models_info.json is a file written to a temporary folder.

Per box on a 24 x 32 frame: the frame, the mask, the box, the canvases squareRGB1 / squareMask1 (padded into a fixed 64 x 64
array; `side` says how much of it is canvas), hs1, centerX / centerY, and KObj for makeNDC False and True.  Once: R, T before
and after the conversion, the diameter and the two depth bounds.

Run from the repo root:  python tests/golden/make_ref_ingest.py
"""
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_from_reference import ref_function, ref_statements                                     # noqa: E402
from make_ref_fields import _save                                                                        # noqa: E402

H, W, MAXB, PAD = 24, 32, 40, 64
#        x, y, w, h, offset
BOXES = ((0, 0, 6, 4, 5),          # in a corner
         (0, 0, 32, 24, 10),       # touching all four edges
         (7, 5, 9, 6, 5),          # odd x even, wider than tall
         (20, 3, 4, 15, 1),        # taller than wide, odd height
         (11, 9, 1, 1, 3),         # one pixel: the even cut leaves nothing
         (3, 2, 13, 11, 0),        # odd x odd, no margin: (K * maxB) / side and K * (maxB / side) round differently here
         (0, 0, 0, 0, 4))          # an empty mask


def main():
    gate = ref_statements("cowrendersynth.py", 667, 667, ("c1[np.where(m1 == 0)] = 0",))
    geometry = ref_statements("cowrendersynth.py", 669, 690, ("if w2 % 2 != 0:", "squareRGB1[hs1 - hh:hs1 + hh, hs1 - hw:hs1 + hw] = c1[y2:y2 + h2, x2:x2 + w2]",
                                                              "centerX = x2 + int(w2 / 2)"))
    cam = ref_statements("cowrendersynth.py", 717, 736, ("camparams = camparams * maxB / squareRGB1.shape[0]", "camparams = camparams * 2 / maxB",
                                                          "KObj[a11][3, 2] = 1"))
    rng = np.random.default_rng(20261021)
    out = {"n_boxes": np.array(len(BOXES), np.int64), "maxB": np.array(MAXB, np.int64)}
    for k, (x, y, w, h, offset) in enumerate(BOXES):
        rgb = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
        mask = np.zeros((H, W, 3), np.uint8)
        if w and h:
            inside = rng.choice(np.array([0, 255], np.uint8), (h, w, 3), p=[0.35, 0.65])
            inside[0, 0, 0] = inside[-1, -1, 0] = inside[0, -1, 0] = inside[-1, 0, 0] = 255
            mask[y:y + h, x:x + w] = inside
        K = np.array([572.4114, 0.0, 325.2611 + rng.uniform(-3, 3), 0.0, 573.57043, 242.04899 + rng.uniform(-3, 3), 0.0, 0.0, 1.0])
        ns = {"np": np, "c1": rgb.copy(), "m1": mask.copy(), "x2": x, "y2": y, "w2": w, "h2": h, "offset": offset, "background": False}
        exec(gate, ns)
        exec(geometry, ns)
        side = ns["squareRGB1"].shape[0]
        assert side <= PAD
        sq, sm = np.zeros((PAD, PAD, 3), np.uint8), np.zeros((PAD, PAD), np.uint8)
        sq[:side, :side], sm[:side, :side] = ns["squareRGB1"], ns["squareMask1"]
        out[f"b{k}_rgb"], out[f"b{k}_mask"], out[f"b{k}_K"] = rgb, mask, K
        out[f"b{k}_box"], out[f"b{k}_offset"] = np.array([x, y, w, h], np.int64), np.array(offset, np.int64)
        out[f"b{k}_canvas_rgb"], out[f"b{k}_canvas_mask"], out[f"b{k}_side"] = sq, sm, np.array(side, np.int64)
        out[f"b{k}_hs1"], out[f"b{k}_center"] = np.array(ns["hs1"], np.int64), np.array([ns["centerX"], ns["centerY"]], np.int64)
        for ndc in (False, True):
            if side == 0:
                continue
            ns.update(camParams={"7": {"cam_K": K.tolist()}}, imId=7, maxB=MAXB, makeNDC=ndc, KObj=np.zeros((1, 4, 4)), a11=0)
            exec(cam, ns)
            out[f"b{k}_KObj_ndc{int(ndc)}"] = ns["KObj"][0].copy()

    # the scripts' first block after the call
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    rotfromeulernp = ref_function("nutil.py", "rotfromeulernp", {"np": np})
    convert = ref_statements("trainNerfFine.py", 91, 101, ("rot180 = rotfromeulernp(np.array([0, 0, np.pi]))", "RObj[a] = RObj[a].T.dot(rot180)",
                                                           "TObj = TObj / scale"))
    bounds = ref_statements("trainNerfFine.py", 118, 119, ("min_depth = np.min(np.abs(TObj[:, 2])) - 2",))
    n = 5
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    T = np.stack([rng.uniform(-80, 80, n), rng.uniform(-80, 80, n), rng.uniform(500, 800, n)], 1)
    diameter = 142.5
    with tempfile.TemporaryDirectory() as tmp:
        (Path(tmp) / "models").mkdir()
        (Path(tmp) / "models" / "models_info.json").write_text(json.dumps({"22": {"diameter": diameter}}))
        ns = {"np": np, "json": json, "rotfromeulernp": rotfromeulernp, "target_images": np.zeros((n, 1)), "RObj": q.copy(), "TObj": T.copy(),
              "datasetPath": tmp, "objid": "22"}
        exec(convert, ns)
        exec(bounds, ns)
    out["pose_R_in"], out["pose_T_in"], out["pose_diameter"] = q, T, np.array(diameter)
    out["pose_R"], out["pose_T"], out["pose_rot180"] = ns["RObj"], ns["TObj"], ns["rot180"]
    out["pose_min_depth"], out["pose_volume_extent_world"] = np.array(ns["min_depth"]), np.array(ns["volume_extent_world"])
    _save("ref_ingest.npz", out)


if __name__ == "__main__":
    main()
