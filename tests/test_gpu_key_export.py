"""GPU: key_export.export_keys on a torus with planted outliers — what is kept is close to the mesh and in FPS order, the
normals, keys and scaled points are what genFeat.py:201-224 states — and the written files feed getCors."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from imagesequenceregistrationfor6dposeestimationlabeling_amd import formats, key_export, ops, registration, synth
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import KeyField
from imagesequenceregistrationfor6dposeestimationlabeling_amd.render import Mesh
from tests import field_ref

pytestmark = pytest.mark.gpu

K, BOX, MAX_DIST, DIAMETER = 2000, 1.2, 0.05, 123.4


class UnitKeys:
    """A field by torch calls: 12 unit-norm channels of random Fourier features and the zero channel the reference's
    batched_customForward appends.  Unit norms make a key its own best match, which the getCors round trip needs."""

    def __init__(self, dev, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.W = (torch.randn(3, 12, generator=g) * 6).to(dev)
        self.b = (torch.rand(12, generator=g) * 6.2831853).to(dev)

    def batched_customForward(self, points, n_batches=16):
        f = torch.nn.functional.normalize(torch.sin(points @ self.W + self.b), dim=-1)
        return torch.cat([f, torch.zeros_like(f[..., :1])], dim=-1)


@pytest.fixture(scope="module")
def scene():
    """A torus of extent about 1 (as the reference's NeRF volume is) and 6 300 candidates in shuffled order: 6 000 surface
    samples with noise 0.01, 200 displaced by 0.2 along the face normal, 100 outside the box."""
    rng = np.random.default_rng(17)
    v, f = synth.make_mesh("torus", 32, radius=0.5 / 1.4, tube=0.4)
    mesh = Mesh(v, f)
    good = synth.sample_surface(v, f, 6000, rng, noise=0.01)
    p, fi = synth.sample_surface(v, f, 200, rng, return_faces=True)
    n = np.cross(v[f[fi, 1]] - v[f[fi, 0]], v[f[fi, 2]] - v[f[fi, 0]])
    off = p + 0.2 * n / np.linalg.norm(n, axis=1, keepdims=True)
    far = synth.sample_surface(v, f, 100, rng)
    far[np.arange(100), rng.integers(0, 3, 100)] = rng.choice([-1.0, 1.0], 100) * rng.uniform(1.2, 2.0, 100)
    cand = np.concatenate([good, off, far]).astype(np.float32)
    perm = rng.permutation(len(cand))
    return dict(mesh=mesh, verts=v, cand=np.ascontiguousarray(cand[perm]), planted=np.nonzero(perm >= 6000)[0])


def _export(scene, dev, field):
    return key_export.export_keys(torch.from_numpy(scene["cand"]).to(dev), scene["mesh"], field, DIAMETER, K=K, box=BOX,
                                  max_dist=MAX_DIST)


def test_export_on_a_torus(cuda0, scene, tmp_path):
    field = UnitKeys(cuda0)
    vert_scaled, feats, normals, kept = _export(scene, cuda0, field)
    N = len(kept)
    print("kept", N, "of", K)
    assert N > 500 and vert_scaled.shape == (N, 3) and feats.shape == (N, 12) and normals.shape == (N, 3)
    assert vert_scaled.dtype == np.float32 and feats.dtype == np.float32 and normals.dtype == np.float64 and kept.dtype == np.int64
    pts = scene["cand"][kept]
    # every kept point is within max_dist of a mesh vertex, and inside the box
    dist, near = cKDTree(scene["verts"]).query(pts.astype(np.float64), k=2)
    assert dist[:, 0].max() < MAX_DIST and np.abs(pts).max() < BOX
    # none of the planted outliers
    assert not set(kept.tolist()) & set(scene["planted"].tolist())
    # a subsequence of the FPS order
    order = ops.fps_sample_host(scene["cand"], K)[0]
    pos = {int(c): i for i, c in enumerate(order)}
    where = [pos[int(c)] for c in kept]                       # KeyError: kept holds a candidate FPS did not select
    assert all(a < b for a, b in zip(where, where[1:]))
    # and everything FPS selected that passes the two filters is kept
    sel = scene["cand"][order].astype(np.float64)
    d_sel = cKDTree(scene["verts"]).query(sel)[0]
    clear = (np.abs(sel).max(1) < BOX) & (np.abs(d_sel - MAX_DIST) > 1e-6)
    assert np.array_equal(order[clear & (d_sel < MAX_DIST)], kept[np.isin(kept, order[clear])])
    # normals: those of the nearest vertex, wherever the nearest is clear
    sure = dist[:, 1] - dist[:, 0] > 1e-6
    assert sure.mean() > 0.9
    assert np.array_equal(normals[sure], scene["mesh"].vertex_normals()[near[sure, 0]])
    # keys: the field called directly on the same points, same bits
    direct = field.batched_customForward(torch.from_numpy(pts).to(cuda0))[..., :-1].cpu().numpy()
    assert np.array_equal(feats.view(np.uint32), direct.view(np.uint32))
    assert np.array_equal(vert_scaled, pts * np.float32(DIAMETER / 1.8))

    # the files, and the first stage that reads them
    formats.save_model(vert_scaled, feats, normals, "UH", "synth", 3, base=tmp_path)
    p2, f2, n2 = formats.load_model("UH", "synth", 3, base=tmp_path)
    assert np.array_equal(p2, vert_scaled) and np.array_equal(f2, feats) and np.array_equal(n2, normals)
    registration.set_surface_points(p2)
    q = np.random.default_rng(4).choice(N, 50, replace=False)
    dots = f2[q].astype(np.float64) @ f2.astype(np.float64).T
    own = dots[np.arange(50), q].copy()
    dots[np.arange(50), q] = -np.inf
    assert (own - dots.max(1)).min() > 1e-5, "the field's keys are not distinct enough for the round trip"
    idx, vals = registration.getCors(torch.from_numpy(f2[q]).to(cuda0), torch.from_numpy(f2).to(cuda0))
    assert np.array_equal(idx.numpy(), q)


def test_export_with_a_key_field_and_few_candidates(cuda0, scene):
    """KeyField is the intended field: its keys are those of a direct call (same bits).  With M < K every candidate is
    sampled, in FPS order."""
    widths, omegas = (3, 64, 64, 12), (30.0, 30.0, None)
    Ws, bs = field_ref.siren_params(widths, omegas, seed=9)
    field = KeyField(Ws, bs, omegas, cuda0)
    few = dict(scene, cand=np.ascontiguousarray(scene["cand"][:900]))
    vert_scaled, feats, normals, kept = _export(few, cuda0, field)
    order = ops.fps_sample_host(few["cand"], 900)[0]
    assert sorted(order.tolist()) == list(range(900))
    pos = {int(c): i for i, c in enumerate(order)}
    where = [pos[int(c)] for c in kept]
    assert len(kept) > 100 and all(a < b for a, b in zip(where, where[1:]))
    pts = few["cand"][kept]
    direct = field.batched_customForward(torch.from_numpy(pts).to(cuda0))[..., :-1].cpu().numpy()
    assert feats.shape == (len(kept), 12) and np.array_equal(feats.view(np.uint32), direct.view(np.uint32))
    assert np.array_equal(vert_scaled, pts * np.float32(DIAMETER / 1.8))
