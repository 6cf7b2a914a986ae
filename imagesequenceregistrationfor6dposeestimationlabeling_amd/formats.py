"""The on-disk hand-offs between the reference's stages, read and written with the
same names and layouts so the surrounding scripts keep working.  Pure host I/O (NumPy / json).

Directory convention of the reference: <UH>_<dataset>_obj_<objid>/  (inference.py:23, choosePose.py:95).
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np


def root_dir(UH, dataset: str, objid) -> Path:
    return Path(f"{UH}_{dataset}_obj_{objid}")


def load_model(UH, dataset: str, objid, base: Path | str = "."):
    """genFeat.py:223-228 outputs: (vert1_scaled (N,3) f32, feat1_scaled (N,D) f32, normals (N,3) f64|None)."""
    d = Path(base) / root_dir(UH, dataset, objid) / f"{objid}poseEst"
    pts = np.load(d / "vert1_scaled.npy").astype(np.float32)
    feats = np.load(d / "feat1_scaled.npy").astype(np.float32)
    nrm = d / "normals_scaled.npy"
    return pts, feats, (np.load(nrm) if nrm.exists() else None)


def save_model(pts, feats, normals, UH, dataset: str, objid, base: Path | str = ".") -> Path:
    """The writer of what load_model reads (genFeat.py:226-228): vert1_scaled.npy (N,3) f32, feat1_scaled.npy (N,D) f32 and,
    unless `normals` is None, normals_scaled.npy (N,3) f64, in <base>/<UH>_<dataset>_obj_<objid>/<objid>poseEst/.
    Returns that directory."""
    pts, feats = np.asarray(pts, np.float32), np.asarray(feats, np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3 or feats.ndim != 2 or feats.shape[0] != pts.shape[0]:
        raise ValueError(f"save_model: pts {pts.shape} and feats {feats.shape}")
    d = Path(base) / root_dir(UH, dataset, objid) / f"{objid}poseEst"
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / "vert1_scaled.npy", pts)
    np.save(d / "feat1_scaled.npy", feats)
    if normals is not None:
        normals = np.asarray(normals, np.float64)
        if normals.shape != pts.shape:
            raise ValueError(f"save_model: normals {normals.shape} for pts {pts.shape}")
        np.save(d / "normals_scaled.npy", normals)
    return d


VIEW_DIRS = ("sampledRayxys", "posVec", "posVecBack", "sampledRayBackxys")      # generateCors.py:358-361, in that order
VIEW_FIELDS = ("xys", "pos_vec", "pos_vec_back", "xys_back")


def save_view_correspondences(nerf_dir: Path | str, render_size: int, view, vc) -> list[Path]:
    """generateCors.py:358-361: the four files of one view, <nerf_dir>/<render_size>_sampledRayxys/<view>.pt (1, n1, 2),
    _posVec (1, n1, 3), _posVecBack (1, n2, 3) and _sampledRayBackxys (1, n2, 2), each a CPU tensor written by torch.save —
    what augment.getNerfSamples loads (augment.py:641-666).  vc: a correspondences.ViewCorrespondences (any object with
    xys, pos_vec, pos_vec_back, xys_back).  Directories are created as needed."""
    import torch
    paths = []
    for sub, name in zip(VIEW_DIRS, VIEW_FIELDS):
        d = Path(nerf_dir) / f"{render_size}_{sub}"
        d.mkdir(parents=True, exist_ok=True)
        t = getattr(vc, name).detach().cpu().contiguous()
        want = 2 if name.startswith("xys") else 3
        if t.ndim != 3 or t.shape[0] != 1 or t.shape[2] != want:
            raise ValueError(f"save_view_correspondences: {name} {tuple(t.shape)} must be (1, n, {want})")
        torch.save(t, d / f"{view}.pt")
        paths.append(d / f"{view}.pt")
    return paths


def load_view_correspondences(nerf_dir: Path | str, render_size: int, view) -> dict:
    """The four files back as augment.py:641-666 reads them -> dict of xys, pos_vec, pos_vec_back, xys_back (CPU tensors)."""
    import torch
    return {name: torch.load(Path(nerf_dir) / f"{render_size}_{sub}" / f"{view}.pt")
            for sub, name in zip(VIEW_DIRS, VIEW_FIELDS)}


def save_subsampled_normals(nerf_dir: Path | str, subvert, subnormal) -> list[Path]:
    """generateCors.py:214-215: <nerf_dir>/subvert1.npy and subnormal1.npy, (K, 3) float32 arrays written by np.save
    (correspondences.subsampled_normals makes them; tensors are copied to the host)."""
    arrays = []
    for name, a in (("subvert", subvert), ("subnormal", subnormal)):
        a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float32)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"save_subsampled_normals: {name} {a.shape} must be (K, 3)")
        arrays.append(a)
    if arrays[0].shape != arrays[1].shape:
        raise ValueError(f"save_subsampled_normals: subvert {arrays[0].shape} and subnormal {arrays[1].shape}")
    Path(nerf_dir).mkdir(parents=True, exist_ok=True)
    paths = [Path(nerf_dir) / "subvert1.npy", Path(nerf_dir) / "subnormal1.npy"]
    for path, a in zip(paths, arrays):
        np.save(path, a)
    return paths


def load_subsampled_normals(nerf_dir: Path | str):
    """The two files back as trainPose.py:196-198 reads them -> (subvert, subnormal), float32 arrays."""
    return (np.load(Path(nerf_dir) / "subvert1.npy").astype("float32"),
            np.load(Path(nerf_dir) / "subnormal1.npy").astype("float32"))


def is_failure(R, t=None) -> bool:
    """pnp()'s failure sentinel is the int triple (1, 1, 1) (inference.py:130-134)."""
    return isinstance(R, (int, np.integer)) or np.ndim(R) == 0


def save_poses(R_list, t_list, UH, dataset: str, objid, base: Path | str = ".", failed: str = "nan"):
    """finalposes.py:234-238 / choosePose.py:303-309 write np.save(pred_R), np.save(pred_t) from Python
    lists — ragged (dtype=object) as soon as one pnp failed.  Here failed images are stored as NaN
    poses (`failed="nan"`, keeps (n,3,3)/(n,3) float64 and the image indexing) or dropped
    (`failed="drop"`); returns the boolean mask of successful images."""
    ok = np.array([not is_failure(R) for R in R_list], bool)
    n = len(R_list)
    R = np.full((n, 3, 3), np.nan)
    t = np.full((n, 3), np.nan)
    for i in range(n):
        if ok[i]:
            R[i], t[i] = np.asarray(R_list[i], np.float64), np.asarray(t_list[i], np.float64).reshape(3)
    if failed == "drop":
        R, t = R[ok], t[ok]
    d = Path(base) / root_dir(UH, dataset, objid)
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / f"{objid}pred_R.npy", R)
    np.save(d / f"{objid}pred_t.npy", t)
    return ok


def load_poses(UH, dataset: str, objid, base: Path | str = "."):
    """choosePose.py:95-96, icp.py:57-58: (pred_R (n,3,3), pred_t (n,3)); tolerates the reference's
    ragged object arrays by mapping sentinel entries to NaN poses."""
    d = Path(base) / root_dir(UH, dataset, objid)
    R = np.load(d / f"{objid}pred_R.npy", allow_pickle=True)
    t = np.load(d / f"{objid}pred_t.npy", allow_pickle=True)
    if R.dtype == object:
        Rn = np.full((len(R), 3, 3), np.nan)
        tn = np.full((len(R), 3), np.nan)
        for i, (a, b) in enumerate(zip(R, t)):
            if not is_failure(a):
                Rn[i], tn[i] = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(3)
        R, t = Rn, tn
    return np.asarray(R, np.float64), np.asarray(t, np.float64)


def write_top_choices(top_indices, UH, dataset: str, objid, base: Path | str = ".") -> Path:
    """choosePose.py:147-150: one image index per line, best first."""
    p = Path(base) / root_dir(UH, dataset, objid) / f"{objid}top_50_choices.txt"
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text("".join(f"{int(i)}\n" for i in top_indices))
    return p


def read_top_choices(UH, dataset: str, objid, base: Path | str = "."):
    """icp.py:37-39."""
    p = Path(base) / root_dir(UH, dataset, objid) / f"{objid}top_50_choices.txt"
    return [int(line.strip()) for line in p.read_text().splitlines() if line.strip()]


def save_vote(error, agreed, UH, dataset: str, objid, base: Path | str = "."):
    """choosePose.py:141-142."""
    d = Path(base) / root_dir(UH, dataset, objid)
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / f"{objid}agreedposes.npy", np.asarray(agreed))
    np.save(d / f"{objid}error.npy", np.asarray(error, np.float64))


def save_relative_poses(table, kind: str, UH, dataset: str, objid, base: Path | str = "."):
    """choosePose.py:111,114: <objid>{gt,pred}_relative_poses.npy, (n,n,4,4) float64."""
    assert kind in ("gt", "pred")
    d = Path(base) / root_dir(UH, dataset, objid)
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / f"{objid}{kind}_relative_poses.npy", np.asarray(table, np.float64))


def write_pred6d_json(R, t, image_ids, path: Path | str):
    """verfication.py:48-52 READS pred6d.json ({img_id: [{"R":[9], "T":[3]}]}) but no script in the
    reference writes it (README.md:92-94 says inference.py does; it does not).  This is the missing
    producer; failed (NaN) poses are skipped."""
    out = {}
    for i, Ri, ti in zip(image_ids, R, t):
        if np.all(np.isfinite(Ri)):
            out[str(int(i))] = [{"R": np.asarray(Ri, np.float64).reshape(9).tolist(),
                                 "T": np.asarray(ti, np.float64).reshape(3).tolist()}]
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(out))
    return out


def read_pred6d_json(path: Path | str):
    """-> (image ids sorted numerically, R (n,3,3), t (n,3)) exactly as verfication.py:50-52, 76-79 index it."""
    d = json.loads(Path(path).read_text())
    keys = sorted(d.keys(), key=lambda x: int(x))
    R = np.array([np.asarray(d[k][0]["R"], np.float64).reshape(3, 3) for k in keys])
    t = np.array([np.asarray(d[k][0]["T"], np.float64) for k in keys])
    return [int(k) for k in keys], R, t


def read_scene_gt(path: Path | str, obj_index: int = 0):
    """BOP scene_gt.json: {img_id: [{"cam_R_m2c":[9], "cam_t_m2c":[3], ...}]} -> ids, R (n,3,3), t (n,3)
    (inference.py:170-186, parsed ONCE instead of once per image)."""
    d = json.loads(Path(path).read_text())
    keys = sorted(d.keys(), key=lambda x: int(x))
    R = np.array([np.asarray(d[k][obj_index]["cam_R_m2c"], np.float64).reshape(3, 3) for k in keys])
    t = np.array([np.asarray(d[k][obj_index]["cam_t_m2c"], np.float64) for k in keys])
    return [int(k) for k in keys], R, t


def read_scene_camera(path: Path | str):
    """BOP scene_camera.json: {img_id: {"cam_K":[9], ...}} -> ids, K (n,3,3)."""
    d = json.loads(Path(path).read_text())
    keys = sorted(d.keys(), key=lambda x: int(x))
    return [int(k) for k in keys], np.array([np.asarray(d[k]["cam_K"], np.float64).reshape(3, 3) for k in keys])


def crop_affine(bbox_xywh, out_size: int = 224, pad: float = 1.2, even_size: bool = True) -> np.ndarray:
    """The 2x3 crop affine M of inference.py:203-219 (host, f64): the bounding box of the visible
    mask (cv2.boundingRect) is shrunk to even width / height (:203-206), then
    size = out/max(w,h)/pad;  M = size * [I | -centre];  M[:,2] += out/2.
    even_size=False skips the decrement for callers that already applied it."""
    x, y, w, h = bbox_xywh
    if even_size:
        if w % 2 != 0:
            w = w - 1
        if h % 2 != 0:
            h = h - 1
    size = out_size / max(w, h) / pad
    c = np.array([x + w / 2.0, y + h / 2.0])
    M = np.concatenate([np.eye(2), -c[:, None]], axis=1) * size
    M[:, 2] += out_size / 2.0
    return M


def crop_camera(K, bbox_xywh, out_size: int = 224, pad: float = 1.2, down_sample: int = 3,
                even_size: bool = True):
    """a4 — the camera-matrix arithmetic of inference.py:203-222 and :260-263 (host, f64):
    cam = [M; 0 0 1] @ K with M = crop_affine(bbox) (odd box sizes are decremented first, exactly as
    the reference does with cv2.boundingRect's output), then the pixel-centre-preserving division
    by the ::down_sample subsampling (camMat[:2,2] += .5; camMat[:2] /= ds; camMat[:2,2] -= .5)."""
    M = crop_affine(bbox_xywh, out_size, pad, even_size)
    cam = np.vstack([M, [0, 0, 1]]) @ np.asarray(K, np.float64)
    cam[:2, 2] += 0.5
    cam[:2] /= down_sample
    cam[:2, 2] -= 0.5
    return cam


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply(path: Path | str):
    """A triangle mesh from an ASCII or binary_little_endian PLY file (what BOP's models/obj_*.ply are) ->
    (vertices (V,3) f64, faces (F,3) i32).  Vertex properties other than x, y, z (normals, colours, texture coordinates) and
    elements other than vertex and face are skipped; a face that is not a triangle raises ValueError."""
    data = Path(path).read_bytes()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []                                 # elements: [name, count, [(prop, type) | (prop, count type, item type)]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if tok[1] == "list":
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii or binary_little_endian)")
    verts = faces = None
    if fmt == "ascii":
        lines = iter(data[body:].decode("ascii").splitlines())
        for name, count, props in elements:
            rows = []
            while len(rows) < count:
                ln = next(lines).split()
                if ln:
                    rows.append(ln)
            if name == "vertex":
                col = [i for want in "xyz" for i, p in enumerate(props) if p[0] == want]
                if len(col) != 3 or any(len(p) != 2 for p in props):
                    raise ValueError(f"{path}: vertex element needs scalar x, y, z")
                verts = np.array([[float(r[c]) for c in col] for r in rows], np.float64).reshape(count, 3)
            elif name == "face":
                if len(props) < 1 or len(props[0]) != 3:
                    raise ValueError(f"{path}: face element needs a leading index list")
                for r in rows:
                    if int(r[0]) != 3:
                        raise ValueError(f"{path}: a face with {int(r[0])} vertices (triangles only)")
                faces = np.array([[int(x) for x in r[1:4]] for r in rows], np.int64).reshape(count, 3)
    else:
        off = body
        for name, count, props in elements:
            if all(len(p) == 2 for p in props):
                dt = np.dtype([(p[0], "<" + p[1]) for p in props])
                block = np.frombuffer(data, dt, count, off)
                off += count * dt.itemsize
                if name == "vertex":
                    if not all(k in dt.names for k in "xyz"):
                        raise ValueError(f"{path}: vertex element needs scalar x, y, z")
                    verts = np.stack([block[k].astype(np.float64) for k in "xyz"], axis=1)
            elif name == "face" and len(props[0]) == 3:
                # triangles make every record the same size: read it as one, and verify the counts
                dt = np.dtype([("n", "<" + props[0][1]), ("idx", "<" + props[0][2], (3,))] +
                              [(p[0], "<" + p[1]) for p in props[1:] if len(p) == 2])
                if any(len(p) == 3 for p in props[1:]):
                    raise ValueError(f"{path}: a second list property on faces is not supported")
                if off + count * dt.itemsize > len(data):
                    raise ValueError(f"{path}: face data is short (triangles only)")
                block = np.frombuffer(data, dt, count, off)
                off += count * dt.itemsize
                if (block["n"] != 3).any():
                    raise ValueError(f"{path}: a face that is not a triangle (triangles only)")
                faces = block["idx"].astype(np.int64)
            else:
                raise ValueError(f"{path}: list property on element {name!r} is not supported")
    if verts is None or faces is None:
        raise ValueError(f"{path}: needs a vertex and a face element")
    if len(faces) and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError(f"{path}: face index outside the {len(verts)} vertices")
    return verts, np.ascontiguousarray(faces, np.int32)
