"""CPU: the host restatement of view_correspondences is assembled from march_host, the brute-force count and an f64 nearest
vertex; the four per-view files round-trip with the reference's shapes and dtypes."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import formats, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
from tests import back_march_ref as br
from tests import density_ref as dr
from tests.back_march_ref import view_rays


def test_host_restatement_composes(hip_lib):
    f = DensityField(*dr.fixture(4, 32, 1, 3), dr.frequencies(4), 10.0, None)
    o, d, ln, xys = view_rays()
    rng = np.random.default_rng(1)
    cloud = np.concatenate([rng.uniform(-1, 1, (3000, 3)), rng.uniform(3, 4, (25, 3))])       # 25 stragglers far from the rest
    keep = br.brute_count(cloud, 0.25, cap=11) > 10                                             # the outlier rule, brute force
    assert keep[:3000].mean() > 0.9 and not keep[3000:].any()
    assert np.array_equal(keep, ops.radius_count_host(cloud, 0.25, cap=11) > 10)
    verts = cloud[keep]
    h = br.view_host(f, o, d, ln, xys, verts, max_dist=0.1)
    n1, n2 = len(h["idx1"]), len(h["idx2"])
    assert 0 < n2 <= n1 <= len(o)
    assert h["xys"].shape == (1, n1, 2) and h["pos_vec"].shape == (1, n1, 3)
    assert h["pos_vec_back"].shape == (1, n2, 3) and h["xys_back"].shape == (1, n2, 2)
    # the back rays start on the front surface, point at the centre line of the origin, and begin at length 0
    assert np.all(h["back_lengths"][:, 0] == 0) and np.allclose(np.linalg.norm(h["back_dirs"], axis=1), 1, atol=1e-6)
    assert np.array_equal(h["back_lengths"], ((ln[h["idx1"]] - ln[h["idx1"]][:, :1]) / np.float32(3.0)).astype(np.float32))
    # the exit point is the LAST sample above 0.05 on the back ray: at or behind the first one
    fr = f.march_host(h["pos_vec"][0], h["back_dirs"], h["back_lengths"], 0.05)
    bk = f.march_host(h["pos_vec"][0], h["back_dirs"], h["back_lengths"], 0.05, direction="back")
    assert np.all(bk["depth"] >= fr["depth"]) and (bk["depth"] > fr["depth"]).any()
    assert np.array_equal(bk["points"], h["back_all"])


def test_files_round_trip_with_the_reference_s_shapes(tmp_path):
    rng = np.random.default_rng(0)
    t = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32))
    vc = SimpleNamespace(xys=t(1, 7, 2), pos_vec=t(1, 7, 3), pos_vec_back=t(1, 4, 3), xys_back=t(1, 4, 2))
    paths = formats.save_view_correspondences(tmp_path / "nerf", 224, 5, vc)
    assert [p.relative_to(tmp_path / "nerf").as_posix() for p in paths] == [
        "224_sampledRayxys/5.pt", "224_posVec/5.pt", "224_posVecBack/5.pt", "224_sampledRayBackxys/5.pt"]
    got = formats.load_view_correspondences(tmp_path / "nerf", 224, 5)
    for k in ("xys", "pos_vec", "pos_vec_back", "xys_back"):
        assert got[k].dtype == torch.float32 and not got[k].is_cuda and torch.equal(got[k], getattr(vc, k)), k
    # augment.py:641-666 indexes them so
    nerf, size, bid = str(tmp_path / "nerf"), 224, 5
    s2 = torch.load(nerf + "/" + str(size) + "_sampledRayBackxys/" + str(bid) + ".pt")[0]
    back = torch.load(nerf + "/" + str(size) + "_posVecBack/" + str(bid) + ".pt")
    s1 = torch.load(nerf + "/" + str(size) + "_sampledRayxys/" + str(bid) + ".pt")[0]
    pos = torch.load(nerf + "/" + str(size) + "_posVec/" + str(bid) + ".pt")
    samps = torch.tensor([2, 0])
    assert s2.shape == (4, 2) and back[:, samps].shape == (1, 2, 3) and s1.shape == (7, 2) and pos[:, samps].shape == (1, 2, 3)
    formats.save_view_correspondences(tmp_path / "nerf", 224, 6, vc)                 # the directories exist now
    with pytest.raises(ValueError):
        formats.save_view_correspondences(tmp_path / "nerf", 224, 7, SimpleNamespace(xys=t(7, 2), pos_vec=t(1, 7, 3),
                                                                                     pos_vec_back=t(1, 4, 3), xys_back=t(1, 4, 2)))
    import imagesequenceregistrationfor6dposeestimationlabeling_amd as pkg
    assert callable(pkg.view_correspondences) and callable(pkg.clean_mesh_vertices)
