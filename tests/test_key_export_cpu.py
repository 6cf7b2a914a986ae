"""CPU: the host pieces of key export — render.Mesh.vertex_normals, synth.sample_surface, formats.save_model — and the
argument checks of sampling / key_export that need no device."""
import numpy as np
import pytest
import torch

import imagesequenceregistrationfor6dposeestimationlabeling_amd as pkg
from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, formats, key_export, sampling, synth
from imagesequenceregistrationfor6dposeestimationlabeling_amd.render import Mesh


def _angle_to(n, r):
    return np.arccos(np.clip((n * r).sum(1), -1.0, 1.0))


def test_vertex_normals_on_a_sphere():
    """Every adjacent face normal of make_mesh("sphere", 8) is within pi/8 of the vertex's radial direction, and a positive
    combination of vectors in a convex cone stays in it."""
    v, f = synth.make_mesh("sphere", 8, winding="ccw")
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    n = Mesh(v, f).vertex_normals()
    assert n.dtype == np.float64 and n.shape == v.shape
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
    assert _angle_to(n, radial).max() < np.pi / 8
    v2, f2 = synth.make_mesh("sphere", 8, winding="cw")
    assert _angle_to(Mesh(v2, f2).vertex_normals(), -radial).max() < np.pi / 8


def test_vertex_normals_are_angle_weighted_and_skip_what_has_no_area():
    # a right-angle corner at the origin in the z = 0 plane and a sliver with a 1-degree corner there in the x = 0 plane
    t = np.radians(1.0)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, np.cos(t), np.sin(t)],
                  [5, 5, 5],                                   # used by no face
                  [2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float64)    # a zero-area face
    f = np.array([[0, 1, 2], [0, 2, 3], [5, 6, 7]], np.int32)
    n = Mesh(v, f).vertex_normals()
    want = (np.pi / 2) * np.array([0, 0, 1.0]) + t * np.array([1.0, 0, 0])
    assert np.allclose(n[0], want / np.linalg.norm(want), atol=1e-12)
    assert np.array_equal(n[4], np.zeros(3)) and np.array_equal(n[5:], np.zeros((3, 3)))
    assert np.array_equal(Mesh(v, np.zeros((0, 3), np.int32)).vertex_normals(), np.zeros_like(v))


def test_sample_surface_is_on_the_surface_and_area_weighted():
    v, f = synth.make_mesh("sphere", 8, radius=1.0)
    rng = np.random.default_rng(0)
    p, fi = synth.sample_surface(v, f, 4000, rng, return_faces=True)
    assert p.shape == (4000, 3) and fi.shape == (4000,)
    r = np.linalg.norm(p, axis=1)
    assert r.max() <= 1 + 1e-12 and r.min() > np.cos(np.pi / 8)
    a, b, c = v[f[fi, 0]], v[f[fi, 1]], v[f[fi, 2]]
    nrm = np.cross(b - a, c - a)
    assert np.abs(((p - a) * nrm).sum(1)).max() < 1e-9           # in its face's plane
    assert abs((p[:, 2] > 0).mean() - 0.5) < 0.05                # the two hemispheres have the same area
    q = synth.sample_surface(v, f, 4000, np.random.default_rng(0), noise=0.01)
    assert 0.005 < np.abs(np.linalg.norm(q, axis=1) - r).std() < 0.02


def test_save_model_then_load_model(tmp_path):
    rng = np.random.default_rng(1)
    pts, feats, nrm = rng.normal(size=(37, 3)), rng.normal(size=(37, 12)), rng.normal(size=(37, 3))
    d = formats.save_model(pts, feats, nrm, "UH", "tless", 5, base=tmp_path)
    assert d == tmp_path / "UH_tless_obj_5" / "5poseEst"
    for name, dt in (("vert1_scaled.npy", np.float32), ("feat1_scaled.npy", np.float32), ("normals_scaled.npy", np.float64)):
        assert np.load(d / name).dtype == dt
    p2, f2, n2 = formats.load_model("UH", "tless", 5, base=tmp_path)
    assert p2.dtype == np.float32 and f2.dtype == np.float32 and n2.dtype == np.float64
    assert np.array_equal(p2, pts.astype(np.float32)) and np.array_equal(f2, feats.astype(np.float32)) and np.array_equal(n2, nrm)
    formats.save_model(pts, feats, None, "UH", "tless", 6, base=tmp_path)
    assert formats.load_model("UH", "tless", 6, base=tmp_path)[2] is None
    with pytest.raises(ValueError):
        formats.save_model(pts, feats[:5], nrm, "UH", "tless", 7, base=tmp_path)


def test_python_surface_refuses_what_it_cannot_do(hip_lib):
    assert pkg.sample_farthest_points is sampling.sample_farthest_points and pkg.thin_keys is sampling.thin_keys
    assert pkg.export_keys is key_export.export_keys
    with pytest.raises(ValueError):
        sampling.sample_farthest_points(torch.zeros(1, 8, 3), K=[2])         # a list of K values
    with pytest.raises(_capi.IsrError):
        sampling.sample_farthest_points(torch.zeros(1, 8, 3), K=2)           # a CPU tensor: no CPU fallback
    with pytest.raises(_capi.IsrError):
        key_export.export_keys(torch.zeros(8, 3), None, None, 1.0)
