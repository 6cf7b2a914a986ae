"""GPU: isr_knn and isr_local_frames against the host build of the same header (which tests/test_knn_cpu.py holds to the
NumPy restatements), bit for bit: the CPU shapes, several workgroups with a ragged last tile at every workgroup width,
reused and poisoned buffers, a caller's stream, rows that do not depend on their companions, non-finite coordinates."""
import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import correspondences, ops, sampling
from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import IsrError
from tests import knn_ref as kr
from tests import poison
from tests.knn_ref import cases, frame_clouds

pytestmark = pytest.mark.gpu
f32 = np.float32


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_rows(got, want):
    (gi, gd), (wi, wd) = got, want
    assert gi.dtype == torch.int32 and gd.dtype == torch.float32
    return np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gd.cpu().numpy().view(np.uint32), wd.view(np.uint32))


def _same_f64(got, want):
    return all(g.dtype == torch.float64 and np.array_equal(g.cpu().numpy().view(np.uint64), w.view(np.uint64)) for g, w in zip(got, want))


@pytest.mark.parametrize("name", list(cases()))
def test_device_rows_equal_the_host_build(cuda0, name):
    q, t, K = cases()[name]
    assert _same_rows(ops.knn(_dev(q, cuda0), _dev(t, cuda0), K), ops.knn_host(q, t, K))


@pytest.fixture(scope="module")
def ragged():
    """65 queries (two workgroups at 16 waves, 17 at 4) over 4 097 targets: four full tiles and one of a single point."""
    rng = np.random.default_rng(41)
    t = rng.normal(0, 0.3, (4097, 3)).astype(f32)
    t[4096] = t[5]                                                  # the last tile's one point ties with an early one
    q = np.concatenate([t[:30], rng.normal(0, 0.3, (35, 3)).astype(f32)])
    return q, t


@pytest.mark.parametrize("K", [1, 64, 65, 1024])
def test_several_workgroups_and_a_ragged_last_tile(cuda0, ragged, K):
    q, t = ragged
    idx, d2 = ops.knn(_dev(q, cuda0), _dev(t, cuda0), K)
    assert _same_rows((idx, d2), ops.knn_host(q, t, K))
    assert ops.knn(_dev(q, cuda0), _dev(t, cuda0), K, want_d2=False)[1] is None
    assert torch.equal(ops.knn(_dev(q, cuda0), _dev(t, cuda0), K, want_d2=False)[0], idx)


def test_k_equal_to_nt_at_1000(cuda0):
    t = np.random.default_rng(43).uniform(-1, 1, (1000, 3)).astype(f32)
    q = t[:9]
    idx, d2 = ops.knn(_dev(q, cuda0), _dev(t, cuda0), 1000)
    assert _same_rows((idx, d2), ops.knn_host(q, t, 1000))
    assert (np.sort(idx.cpu().numpy(), axis=1) == np.arange(1000)).all()


def test_a_row_does_not_depend_on_its_companions(cuda0, ragged):
    _, t = ragged
    td = _dev(t, cuda0)
    for K in (7, 300, 1000):                                         # 16, 8 and 4 waves per workgroup
        batch = ops.knn(td, td, K)
        for i in (0, 15, 16, 4096):
            alone = ops.knn(td[i:i + 1], td, K)
            assert torch.equal(alone[0][0], batch[0][i]) and torch.equal(alone[1][0].view(torch.int32), batch[1][i].view(torch.int32))


@pytest.mark.parametrize("name", ["torus, K = 20", "1000 FPS points, K = 400"])
def test_device_frames_equal_the_host_build(cuda0, name):
    pts, K = frame_clouds()[name]
    idx = ops.knn_host(pts, pts, K)[0]
    pd, idd = _dev(pts, cuda0), _dev(idx, cuda0)
    assert torch.equal(ops.knn(pd, pd, K, want_d2=False)[0], idd)
    for dis in (False, True):
        assert _same_f64(ops.local_frames(pd, idd, dis), ops.local_frames_host(pts, idx, dis))


def test_identical_cloud_on_the_device(cuda0):
    pts = np.tile(np.array([[0.1, 0.2, 0.3]], f32), (33, 1))
    pd = _dev(pts, cuda0)
    idx = ops.knn(pd, pd, 7)[0]
    assert (idx.cpu().numpy() == np.arange(7)).all()
    for dis in (False, True):
        got = ops.local_frames(pd, idx, dis)
        assert _same_f64(got, ops.local_frames_host(pts, idx.cpu().numpy(), dis))
    assert (got[0] == 0).all() and torch.equal(got[1].cpu(), torch.diag(torch.tensor([-1.0, 1.0, -1.0], dtype=torch.float64)).expand(33, 3, 3))


def test_reused_and_poisoned_buffers_and_a_callers_stream(cuda0, monkeypatch):
    big, K_big = frame_clouds()["torus, K = 50"]
    q, t, K = cases()["Nt = 257, K = 64"]
    bd, qd, td = _dev(big, cuda0), _dev(q, cuda0), _dev(t, cuda0)

    def run():
        first = ops.knn(bd, bd, K_big)
        second = ops.knn(qd, td, K)                                  # the same cached workspace
        third = ops.knn(bd, bd, 600, want_d2=False)[0]
        frames = ops.local_frames(bd, first[0])
        again = ops.local_frames(bd, first[0])                       # a second call
        return first, second, third, frames, again

    a, b = poison.run_twice(monkeypatch, run)
    assert poison.same_bits(a, b) and poison.same_bits(a[3], a[4])
    assert _same_rows(a[0], ops.knn_host(big, big, K_big)) and _same_rows(a[1], ops.knn_host(q, t, K))
    assert np.array_equal(a[2].numpy(), ops.knn_host(big, big, 600)[0])
    assert _same_f64(a[3], ops.local_frames_host(big, a[0][0].numpy()))
    side = torch.cuda.Stream(device=cuda0)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        on_side = ops.knn(bd, bd, K_big)
        frames_side = ops.local_frames(bd, on_side[0])
    side.synchronize()
    assert poison.same_bits(poison.to_host(on_side), a[0]) and poison.same_bits(poison.to_host(frames_side), a[3])
    ops.clear_workspaces()


def test_non_finite_coordinates_stay_inside(cuda0):
    rng = np.random.default_rng(47)
    cloud = rng.normal(size=(1500, 3)).astype(f32)
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = cloud.copy()
        bad[rng.choice(1500, 40, replace=False), rng.integers(0, 3, 40)] = bad_value
        bd = _dev(bad, cuda0)
        with pytest.raises(ValueError):
            ops.knn(bd, bd, 5)
        for K in (5, 700):
            idx, d2 = ops.knn(bd, bd, K, check_finite=False)
            torch.cuda.synchronize()
            got = idx.cpu().numpy()
            assert got.shape == (1500, K) and got.min() >= 0 and got.max() < 1500
        curv, frames = ops.local_frames(bd, idx[:, :30].contiguous())           # unspecified values, no access outside
        torch.cuda.synchronize()
        assert curv.shape == (1500, 3) and frames.shape == (1500, 3, 3)


def test_normals_with_pytorch3d_call_shapes(cuda0):
    torus, K = frame_clouds()["torus, K = 20"]
    td = _dev(torus, cuda0)
    curv, frames = sampling.estimate_pointcloud_local_coord_frames(td, K)
    want = sampling.estimate_pointcloud_local_coord_frames(torus, K, host=True)
    assert curv.dtype == frames.dtype == torch.float32 and curv.device == td.device
    assert np.array_equal(curv.cpu().numpy(), want[0]) and np.array_equal(frames.cpu().numpy(), want[1])
    both = torch.stack([td[:300], td[300:600]])
    nb = sampling.estimate_pointcloud_normals(both, neighborhood_size=12)
    assert nb.shape == (2, 300, 3)
    assert np.array_equal(nb.cpu().numpy(), sampling.estimate_pointcloud_normals(both.cpu().numpy(), 12, host=True))
    with pytest.raises(ValueError):
        sampling.estimate_pointcloud_normals(td, neighborhood_size=900)
    with pytest.raises(IsrError):
        sampling.estimate_pointcloud_normals(td.cpu(), neighborhood_size=20)


def test_subsampled_normals_equal_the_host_entries(cuda0):
    cloud = kr.surface_cloud("torus", 2000, 9).astype(np.float64)
    want = correspondences.subsampled_normals(cloud, K=300, neighborhood_size=120, host=True)
    got = correspondences.subsampled_normals(torch.from_numpy(cloud).to(cuda0), K=300, neighborhood_size=120)
    assert got[0].dtype == got[1].dtype == torch.float32 and got[0].device == cuda0
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    as_numpy = correspondences.subsampled_normals(cloud, K=300, neighborhood_size=120)
    assert as_numpy[0].dtype == as_numpy[1].dtype == f32
    assert np.array_equal(as_numpy[0], want[0]) and np.array_equal(as_numpy[1], want[1])
    with pytest.raises(ValueError):
        correspondences.subsampled_normals(torch.from_numpy(cloud[:299]).to(cuda0), K=300, neighborhood_size=120)


def test_refusals_on_the_device(cuda0):
    pts = torch.zeros(4, 3, device=cuda0)
    for K in (0, 5, 1025):
        with pytest.raises(ValueError):
            ops.knn(pts, pts, K)
    with pytest.raises(ValueError):
        ops.knn(torch.zeros(0, 3, device=cuda0), pts, 1)
    with pytest.raises(ValueError):
        ops.knn(pts, torch.zeros(4, 2, device=cuda0), 1)
    with pytest.raises(IsrError):
        ops.knn(torch.zeros(4, 3), pts, 1)
    with pytest.raises(ValueError):
        ops.local_frames(pts, torch.zeros(3, 2, dtype=torch.int32, device=cuda0))
    from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import current_stream, lib, ptr
    idx = torch.zeros(4, 2, dtype=torch.int32, device=cuda0)
    ws = torch.zeros(8, dtype=torch.uint8, device=cuda0)
    rc = lib().isr_knn(ptr(pts), 4, ptr(pts), 4, 2, ptr(idx), None, ptr(ws), ws.numel(), current_stream(cuda0))
    assert rc == -1 and b"workspace" in lib().isr_last_error()
