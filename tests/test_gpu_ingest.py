"""GPU: the sequence ingest (include/isr_ingest.h).  The device against the library's host build, bit for bit, on every case of
tests/test_ingest_cpu.py's sweep with the outputs and the workspace pre-filled between guard bands; the tiling edges of the
three kernels; one realistic chunk; ingest.training_views feeding the ray sampler and augment.PoseBatches."""
import numpy as np
import pytest
import torch

from tests import ingest_ref as ir
from tests import poison

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x7F)      # what the outputs and the workspace hold before the call
GUARD_BYTE, GUARD = 0xA5, 256
NAMES = ("images", "silhouettes", "K", "geom", "status")
SIL = {"linear": 0, "nearest": 1}


def same(a, b):
    """Bit equality of a device result with the host's: NaN matches NaN of the same bits, -0.0 is not +0.0."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return ir.same(a, np.asarray(b))


def _mods():
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
    return _capi.lib(), ops


def guarded(dev, rgb_d, mask_d, K_d, max_b, offset, make_ndc, silhouette, fill, ws_bytes=None, stream=None):
    """isr_ingest_views through the C ABI into one buffer: guard | images | guard | silhouettes | guard | K | guard | geom | guard |
    status | guard | workspace | guard, the carves pre-filled with `fill`.  -> (rc, the five outputs as host arrays, guards intact)."""
    L, ops = _mods()
    n, H, W, _ = rgb_d.shape
    Cm, B = mask_d.shape[3], max(int(max_b), 0)
    B = B if B <= 4096 else 1      # a refused size: nothing is written, nothing that large is allocated
    need = ops.ingest_workspace_bytes(n, H, W, Cm) if ws_bytes is None else ws_bytes
    sizes = [n * B * B * 12, n * B * B * 4, n * 128, n * 32, n * 4, max(need, 16)]
    offs, o = [], GUARD
    for s in sizes:
        offs.append(o)
        o = (o + s + GUARD + 255) // 256 * 256
    buf = torch.full((o,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    for a, s in zip(offs, sizes):
        buf[a:a + s] = fill
    p = [buf.data_ptr() + a for a in offs]
    st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream.cuda_stream
    rc = L.isr_ingest_views(rgb_d.data_ptr(), mask_d.data_ptr(), K_d.data_ptr(), n, H, W, Cm, int(max_b), int(offset), int(make_ndc),
                            SIL.get(silhouette, silhouette), p[0], p[1], p[2], p[3], p[4], p[5], need, st)
    if stream is not None:
        stream.synchronize()
    host = buf.cpu().numpy()
    keep = np.ones(o, bool)
    for a, s in zip(offs[:5], sizes[:5]):
        keep[a:a + s] = False
    keep[offs[5]:offs[5] + sizes[5]] = False
    intact = bool((host[keep] == GUARD_BYTE).all())
    cut = lambda k, dt, shape: host[offs[k]:offs[k] + sizes[k]].view(dt).reshape(shape).copy()
    out = (cut(0, np.float32, (n, B, B, 3)), cut(1, np.float32, (n, B, B)), cut(2, np.float64, (n, 4, 4)), cut(3, np.int32, (n, 8)),
           cut(4, np.int32, (n,)))
    return rc, out, intact


def upload(dev, b):
    return (torch.from_numpy(np.ascontiguousarray(b["rgb"])).to(dev), torch.from_numpy(np.ascontiguousarray(b["mask"])).to(dev),
            torch.from_numpy(np.ascontiguousarray(b["K"], np.float64)).to(dev))


def check_against_host(dev, b, fill, dev_arrays=None):
    L, ops = _mods()
    r, m, K = dev_arrays if dev_arrays is not None else upload(dev, b)
    rc, got, intact = guarded(dev, r, m, K, b["max_b"], b["offset"], b["make_ndc"], b["silhouette"], fill)
    what = f"{tuple(b['rgb'].shape)} Cm={b['mask'].shape[3]} maxB={b['max_b']} offset={b['offset']} ndc={b['make_ndc']} {b['silhouette']} fill={fill:#x}"
    assert rc == 0, f"{what}: {L.isr_last_error()}"
    assert intact, f"{what}: a guard band was written"
    ref = ops.ingest_views_host(**b)
    bad = [nm for nm, g, h in zip(NAMES, got, ref) if not ir.same(g, h)]
    assert not bad, f"{what}: {bad} differ from the host build"
    return got


# ---------------------------------------------------------------- 1. the sweep
@pytest.mark.parametrize("Cm", (1, 3))
@pytest.mark.parametrize("H,W", ir.SIZES)
def test_device_equals_host_on_the_sweep(cuda0, H, W, Cm):
    rgb, mask, K, _ = ir.frames(H, W, Cm)
    full = upload(cuda0, dict(rgb=rgb, mask=mask, K=K))
    for j, b in enumerate(ir.batches(H, W, Cm)):
        n = b["rgb"].shape[0]
        # slices of the uploaded batch: their frames start at addresses that are not 16-aligned
        arrays = full if n == ir.N_FRAMES else None
        if n == 2:
            arrays = tuple(t[2:4] for t in full)
        check_against_host(cuda0, b, FILLS[j % 3], arrays)


@pytest.mark.parametrize("fill", FILLS)
def test_every_fill_on_one_batch(cuda0, fill):
    rgb, mask, K, _ = ir.frames(17, 33, 3)
    for sil in ("linear", "nearest"):
        got = check_against_host(cuda0, dict(rgb=rgb, mask=mask, K=K, max_b=7, offset=0, make_ndc=True, silhouette=sil), fill)
        assert got[4].sum() >= 1 and np.isnan(got[2][got[4] == 1]).all() and not got[0][got[4] == 1].view(np.uint32).any()


def test_wrapper_second_call_reused_workspace_and_stream(cuda0, monkeypatch):
    L, ops = _mods()
    rgb, mask, K, _ = ir.frames(33, 17, 3)
    b = dict(rgb=rgb, mask=mask, K=K, max_b=33, offset=1, make_ndc=False, silhouette="linear")
    ref = ops.ingest_views_host(**b)
    r, m, Kd = upload(cuda0, b)

    def run():
        first = ops.ingest_views(r, m, Kd, 33, 1, False, "linear")
        second = ops.ingest_views(r, m, Kd, 33, 1, False, "linear")      # the cached workspace again
        return tuple(first), tuple(second)

    for res in poison.run_twice(monkeypatch, run):
        for call in res:
            assert all(same(g, h) for g, h in zip(call, ref))
    # a caller's workspace, poisoned, and a caller's stream
    ws = torch.full((ops.ingest_workspace_bytes(17, 33, 17, 3),), 0x7F, dtype=torch.uint8, device=cuda0)
    s = torch.cuda.Stream(cuda0)
    s.wait_stream(torch.cuda.current_stream(cuda0))
    with torch.cuda.stream(s):
        got = ops.ingest_views(r, m, Kd, 33, 1, False, "linear", workspace_buf=ws)
    s.synchronize()
    assert all(same(g, h) for g, h in zip(got, ref))
    rc, got2, intact = guarded(cuda0, r, m, Kd, 33, 1, False, "linear", 0xFF, stream=s)
    assert rc == 0 and intact and all(ir.same(g, h) for g, h in zip(got2, ref))
    # mask (n, H, W) without a channel axis is one channel
    got = ops.ingest_views(r, m[..., 0].contiguous(), Kd, 9, 5, True, "nearest")
    assert all(same(g, h) for g, h in zip(got, ops.ingest_views_host(rgb, mask[..., 0], K, 9, 5, True, "nearest")))


def test_refusals_write_nothing(cuda0):
    L, ops = _mods()
    from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import IsrError
    rgb, mask, K, _ = ir.frames(5, 8, 3)
    r, m, Kd = upload(cuda0, dict(rgb=rgb, mask=mask, K=K))
    ok = dict(max_b=4, offset=2, make_ndc=1, silhouette=0)
    for change in (dict(max_b=0), dict(max_b=4097), dict(offset=-1), dict(offset=4097), dict(silhouette=2), dict(silhouette=-1)):
        rc, got, intact = guarded(cuda0, r, m, Kd, fill=0x7F, **{**ok, **change})
        assert rc == -1 and L.isr_last_error(), change
        assert intact and all((g.view(np.uint8) == 0x7F).all() for g in got if g.size), change
    rc, got, intact = guarded(cuda0, r, m[..., :2].contiguous(), Kd, fill=0x7F, ws_bytes=4096, **ok)
    assert rc == -1 and b"Cm" in L.isr_last_error() and all((g.view(np.uint8) == 0x7F).all() for g in got)
    rc, got, intact = guarded(cuda0, r, m, Kd, fill=0x7F, ws_bytes=ops.ingest_workspace_bytes(17, 5, 8, 3) - 1, **ok)
    assert rc == -1 and b"workspace" in L.isr_last_error() and all((g.view(np.uint8) == 0x7F).all() for g in got)
    out = [torch.full((256,), 0x7F, dtype=torch.uint8, device=cuda0) for _ in range(6)]
    p = [t.data_ptr() for t in out]
    st = torch.cuda.current_stream(cuda0).cuda_stream
    args = lambda **kw: (kw.get("rgb", r.data_ptr()), kw.get("mask", m.data_ptr()), kw.get("K", Kd.data_ptr()), kw.get("n", 1), kw.get("H", 1),
                         kw.get("W", 1), 3, 1, 0, 0, 0, kw.get("images", p[0]), p[1], p[2], p[3], kw.get("status", p[4]), kw.get("ws", p[5]), 256, st)
    assert L.isr_ingest_views(*args()) == 0
    torch.cuda.synchronize()
    for t in out:
        t.fill_(0x7F)
    for kw in (dict(rgb=None), dict(mask=None), dict(K=None), dict(images=None), dict(status=None), dict(ws=None), dict(ws=p[5] + 4), dict(n=0),
               dict(n=64 * 65535 + 1), dict(H=0), dict(W=0), dict(H=1 << 14, W=(1 << 14) + 1)):
        assert L.isr_ingest_views(*args(**kw)) == -1 and L.isr_last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((t == 0x7F).all()) for t in out)
    with pytest.raises(IsrError):
        ops.ingest_views(r.cpu(), m, Kd, 4)
    with pytest.raises(ValueError):
        ops.ingest_views(r.float(), m, Kd, 4)
    with pytest.raises(ValueError, match="silhouette"):
        ops.ingest_views(r, m, Kd, 4, silhouette="cubic")


# ---------------------------------------------------------------- 2. the tiling edges
def _blob_frames(n, H, W, Cm, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(1, 256, (n, H, W, 3), dtype=np.uint8)
    mask = np.zeros((n, H, W, Cm), np.uint8)
    for i in range(n):
        x0, x1 = sorted(rng.integers(0, W, 2))
        y0, y1 = sorted(rng.integers(0, H, 2))
        mask[i, y0:y1 + 1, x0:x1 + 1] = rng.choice(np.array([0, 255], np.uint8), (y1 - y0 + 1, x1 - x0 + 1, Cm), p=[0.5, 0.5])
        mask[i, y0, x1, 0] = mask[i, y1, x0, 0] = 255
    K = np.tile(np.array([572.4114, 0.0, W / 2, 0.0, 573.57043, H / 2, 0.0, 0.0, 1.0]), (n, 1))
    return rgb, mask, K


@pytest.mark.parametrize("Cm", (1, 3))
def test_more_rows_than_one_strip_with_a_ragged_last_strip(cuda0, Cm):
    L, ops = _mods()
    rows, strips = ops.ingest_strips(257, 19, Cm)
    assert strips > 1 and 257 % rows != 0
    rgb, mask, K = _blob_frames(5, 257, 19, Cm, 1)
    mask[3] = 0
    mask[3, 256, 18, 0] = mask[3, 256, 3, 0] = mask[3, 250, 9, 0] = 7      # the box ends in the last, short strip
    mask[4] = 0
    mask[4, 0, 0, 0] = mask[4, rows, 18, 0] = 1                            # first byte of the frame, first row of the second strip
    got = check_against_host(cuda0, dict(rgb=rgb, mask=mask, K=K, max_b=31, offset=3, make_ndc=True, silhouette="linear"), 0xFF)
    assert got[3][3].tolist()[:4] == [3, 250, 16, 6] and got[3][4].tolist()[:4] == [0, 0, 18, rows]


@pytest.mark.parametrize("Cm", (1, 3))
def test_a_row_longer_than_a_workgroups_span(cuda0, Cm):
    L, ops = _mods()
    assert 4099 * Cm > 256 * 16 and ops.ingest_strips(3, 4099, Cm)[1] >= 1
    rgb, mask, K = _blob_frames(3, 3, 4099, Cm, 2)
    mask[2] = 0
    mask[2, 0, 4098, 0] = mask[2, 2, 4097, 0] = 255                        # only the row's last bytes
    got = check_against_host(cuda0, dict(rgb=rgb, mask=mask, K=K, max_b=40, offset=0, make_ndc=False, silhouette="nearest"), 0x7F)
    assert got[3][2].tolist()[:4] == [4097, 0, 2, 2]


def test_more_frames_than_one_group_and_a_partial_resize_workgroup(cuda0):
    L, ops = _mods()
    geo = ops.ingest_geometry()
    assert 65 > geo["frame_group"] and (17 * 17) % geo["threads"] != 0
    rgb, mask, K = _blob_frames(65, 9, 11, 3, 3)
    K[:, 2] += np.arange(65)
    got = check_against_host(cuda0, dict(rgb=rgb, mask=mask, K=K, max_b=17, offset=2, make_ndc=True, silhouette="linear"), 0xFF)
    assert got[0][64].any()


# ---------------------------------------------------------------- 3. one realistic chunk
def test_realistic_chunk_equals_host_and_repeats(cuda0):
    L, ops = _mods()
    n, H, W = 16, 480, 640
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.zeros((n, H, W, 3), np.uint8)
    for i in range(n):
        cx, cy, rad = rng.integers(150, 490), rng.integers(120, 360), rng.integers(40, 110)
        mask[i][(xx - cx) ** 2 + (yy - cy) ** 2 <= rad ** 2] = 255
    K = np.tile(np.array([572.4114, 0.0, 325.2611, 0.0, 573.57043, 242.04899, 0.0, 0.0, 1.0]), (n, 1))
    r, m, Kd = upload(cuda0, dict(rgb=rgb, mask=mask, K=K))
    a = ops.ingest_views(r, m, Kd, 224, 5, False, "linear")
    b = ops.ingest_views(r, m, Kd, 224, 5, False, "linear")
    ref = ops.ingest_views_host(rgb, mask, K, 224, 5, False, "linear")
    for nm, x, y, h in zip(NAMES, a, b, ref):
        assert same(x, h), f"{nm} differs from the host build"
        assert same(y, x.cpu().numpy()), f"{nm}: two calls give different bytes"
    assert int(a.status.sum()) == 0 and float(a.silhouettes.mean()) > 0.3


# ---------------------------------------------------------------- 4. training_views downstream
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("bop")
    rgb, mask, K, R, T = ir.folder_frames(4, H=24, W=32)
    ir.write_bop_tree(root, rgb, mask, K, R, T, objid="22")
    return root, rgb, mask, K, R, T


def test_training_views_feed_the_ray_sampler(cuda0, tree):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ingest, rays
    root, rgb, mask, K, R, T = tree
    v = ingest.training_views(str(root), "22", "tless", 1, max_b=16, device=cuda0, ids=range(4), chunk=3)
    assert v.images.is_cuda and v.images.dtype == torch.float32 and tuple(v.images.shape) == (4, 16, 16, 3)
    host = ingest.training_views(str(root), "22", "tless", 1, max_b=16, device="cpu", ids=range(4))
    assert same(v.images, host.images.numpy()) and same(v.silhouettes, host.silhouettes.numpy()) and ir.same(v.K, host.K)
    assert ir.same(v.R, host.R) and ir.same(v.T, host.T) and v.min_depth == host.min_depth
    idx = [0, 2]
    cams = v.cameras(idx, 16, in_ndc=False)
    sampler = rays.NDCMultinomialRaysampler(image_width=16, image_height=16, n_pts_per_ray=8, min_depth=v.min_depth, max_depth=v.volume_extent_world)
    bundle = sampler(cams, mask=v.silhouettes[idx, ..., None])
    assert isinstance(bundle, rays.RayBundle) and bundle.origins.is_cuda
    count = int((v.silhouettes[idx] != 0).sum())
    assert tuple(bundle.origins.shape) == (1, count, 3) and tuple(bundle.lengths.shape) == (1, count, 8) and count > 0
    # the drop-in on the device returns CPU tensors, the same bits
    out = ingest.generate_bop_realsamples(str(root), "22", maxB=16, offset=5, synth=False, makeNDC=False, device=cuda0, chunk=3)
    assert not out[0].is_cuda and same(out[0], host.images.numpy()) and ir.same(out[4], host.K)


def test_pose_batches_accept_nearest_silhouettes(cuda0, tree):
    """augment.PoseBatches needs 0/1 silhouettes (augment.py:299 of the reference's generateImages).  "nearest" over a 0/255 mask
    gives them.  "linear" does not raise there either: its fractional edge values are truncated to 0 by PoseBatches'
    .to(uint8), so the mask loses its soft rim — PoseBatches' own, unchanged behaviour, stated in INTEGRATION §28."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import augment, ingest
    root, rgb, mask, K, R, T = tree
    v = ingest.training_views(str(root), "22", "tless", 1, max_b=16, device=cuda0, ids=range(4), silhouette="nearest")
    assert set(torch.unique(v.silhouettes).tolist()) == {0.0, 1.0}
    rng = np.random.default_rng(3)
    vs = [{"xys": torch.from_numpy(rng.uniform(-0.6, 0.6, (1, 90, 2)).astype(np.float32)), "pos_vec": torch.from_numpy(rng.uniform(-1, 1, (1, 90, 3)).astype(np.float32)),
           "pos_vec_back": torch.from_numpy(rng.uniform(-1, 1, (1, 70, 3)).astype(np.float32)), "xys_back": torch.from_numpy(rng.uniform(-0.6, 0.6, (1, 70, 2)).astype(np.float32))}
          for _ in range(4)]
    bank = augment.CorrespondenceBank.from_views(vs, cuda0)
    batches = augment.PoseBatches(v.images, v.silhouettes, bank, batch_size=2, sample_size=32, seed=1)
    assert torch.equal(batches.masks, v.silhouettes.to(torch.uint8))
    rgb_b, mask_b, pos, xys, extras = next(iter(batches))
    assert tuple(rgb_b.shape) == (2, 16, 16, 3) and tuple(mask_b.shape) == (2, 16, 16) and tuple(pos.shape) == (2, 32, 3)
    lin = ingest.training_views(str(root), "22", "tless", 1, max_b=16, device=cuda0, ids=range(4), silhouette="linear")
    frac = (lin.silhouettes > 0) & (lin.silhouettes < 1)
    assert bool(frac.any())
    soft = augment.PoseBatches(lin.images, lin.silhouettes, bank, batch_size=2, sample_size=32, seed=1)
    assert torch.equal(soft.masks, (lin.silhouettes == 1).to(torch.uint8)) and not bool(soft.masks[frac].any())
