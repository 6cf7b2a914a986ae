"""GPU: isr_augment_images and isr_augment_rays against the host build of the same header (which tests/test_augment_cpu.py holds
to the NumPy restatement of include/isr_augment.h), bit for bit with NaN-aware equality, on every case of the CPU tests; one
16 x 224 x 224 batch; views of 4 097 and 50 176 rows at S = 1 024 and 4 096; outputs pre-filled with 0x00, 0xFF and 0x7F; a
second call and a caller's stream; each optional input left out; the refusals; and augment.PoseBatches into three
training.pose_train_step's."""
import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, augment, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import TrainableKeyField
from imagesequenceregistrationfor6dposeestimationlabeling_amd.training import pose_train_step
from tests import augment_ref as ar
from tests import poison

pytestmark = pytest.mark.gpu
f32 = np.float32

FILLS = (0x00, 0xFF, 0x7F)                    # what the outputs hold before the call (there is no workspace)
IMAGE_CASES = ar.image_cases()
RAY_CASES = ar.ray_cases()


def same(a, b):
    """Bit equality of an f32 / i32 device result with the host's, a NaN matching any NaN."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def dev_images(dev, kw):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(kw)
    for k in ("rgb", "mask", "orig_mask", "canvas"):
        if k in d:
            d[k] = t(d[k])
    return d


def dev_bank(dev, bank):
    return None if bank is None else (torch.from_numpy(bank[0]).to(dev), torch.from_numpy(bank[1]).to(dev), bank[2])


def check_rays(got, want, what):
    for name in ("xys", "pos", "index", "count"):
        assert same(getattr(got, name), getattr(want, name)), f"{what}: {name}"


# ---------------------------------------------------------------- images
@pytest.mark.parametrize("name", [c[0] for c in IMAGE_CASES])
def test_images_device_against_host(cuda0, monkeypatch, name):
    kw = dict(IMAGE_CASES)[name]
    want = ops.augment_images_host(**kw)
    d = dev_images(cuda0, kw)
    for byte in FILLS:
        with poison.poisoned(monkeypatch, byte):
            got = poison.to_host(ops.augment_images(**d))
        for what, g, w in zip(("rgb_out", "mask_orig_out", "mask_out"), got, want):
            assert same(g, w), f"{name}: fill {byte:#x} {what}"


def test_images_training_batch_second_call_and_stream(cuda0):
    """16 x 224 x 224 with canvases, rectangles, shifts and border kernels: device against host; a second call; a caller's stream."""
    B, H = 16, 224
    rng = np.random.default_rng(16)
    rgb, mask, orig, canvas = ar.image_inputs(rng, B, H, H)
    mask[:, 40:180, 50:170] = 1
    bbox = np.array([[50, 40, 120, 140]] * B)
    p = augment.draw_params(B, 3, H, bbox=bbox, integral=augment.mask_integral(torch.from_numpy(mask)), borderADD=True, maskMax=100)
    p.border[:3] = torch.tensor([[19, 19], [2, 3], [1, 1]], dtype=torch.int32)
    kw = dict(rgb=rgb, mask=mask, M=p.M.numpy(), orig_mask=orig, canvas=canvas, rect=p.rect.numpy(), tra=p.tra.numpy(), tra1=p.tra1.numpy(),
              border=p.border.numpy())
    want = ops.augment_images_host(**kw)
    assert want[2].mean() > 0.05 and (p.rect[:, 2] > 0).any()
    d = dev_images(cuda0, kw)
    first = ops.augment_images(**d)
    second = ops.augment_images(**d)
    stream = torch.cuda.Stream(device=cuda0)
    stream.wait_stream(torch.cuda.current_stream(cuda0))
    with torch.cuda.stream(stream):
        third = ops.augment_images(**d)
    stream.synchronize()
    for got in (first, second, third):
        for what, g, w in zip(("rgb_out", "mask_orig_out", "mask_out"), got, want):
            assert same(g, w), what


def test_images_pixels_no_multiple_of_the_workgroup(cuda0):
    """H W = 17 x 19 = 323 = 256 + 67 and 1 x 257: a partial last workgroup; more than 16 images: a second launch group."""
    rng = np.random.default_rng(5)
    for B, H, W in ((18, 17, 19), (1, 1, 257)):
        rgb, mask, orig, canvas = ar.image_inputs(rng, B, H, W)
        M = np.stack([ar.rotation(W, H, 10 * b + 3, 0.9) for b in range(B)])
        kw = dict(rgb=rgb, mask=mask, M=M, orig_mask=orig, canvas=canvas, tra=rng.integers(-3, 4, (B, 2)), tra1=rng.integers(-3, 4, (B, 2)),
                  border=np.tile([[3, 4]], (B, 1)))
        for g, w in zip(ops.augment_images(**dev_images(cuda0, kw)), ops.augment_images_host(**kw)):
            assert same(g, w)


def test_images_optional_inputs(cuda0):
    """Each optional input left out alone, and all of them; orig_mask left out is the mask itself (the same pointer)."""
    rng = np.random.default_rng(6)
    B, H, W = 2, 9, 12
    rgb, mask, orig, canvas = ar.image_inputs(rng, B, H, W)
    M = np.stack([ar.rotation(W, H, 20, 1.1)] * B)
    full = dict(orig_mask=orig, canvas=canvas, rect=np.array([[2, 2, 4, 3]] * B), tra=np.array([[1, 2]] * B), tra1=np.array([[-1, 0]] * B),
                border=np.array([[2, 2]] * B))
    for drop in (*full, None):
        opt = {k: v for k, v in full.items() if k != drop} if drop else {}
        kw = dict(rgb=rgb, mask=mask, M=M, **opt)
        for g, w in zip(ops.augment_images(**dev_images(cuda0, kw)), ops.augment_images_host(**kw)):
            assert same(g, w), drop


# ---------------------------------------------------------------- rays
@pytest.mark.parametrize("name", [c[0] for c in RAY_CASES])
def test_rays_device_against_host(cuda0, monkeypatch, name):
    _, front, back, ids, rot, t, S, seed = next(c for c in RAY_CASES if c[0] == name)
    want = ops.augment_rays_host(front, ids, rot, t, S, seed, back=back)
    f, b = dev_bank(cuda0, front), dev_bank(cuda0, back)
    for byte in FILLS:
        with poison.poisoned(monkeypatch, byte):
            got = poison.to_host(ops.augment_rays(f, ids, rot, t, S, seed, back=b))  # a dataclass comes back as a dict
        for s, (g, w) in enumerate(zip((got,) if back is None else got, (want,) if back is None else want)):
            for k in ("xys", "pos", "index", "count"):
                assert same(g[k], getattr(w, k)), f"{name}: fill {byte:#x} set {s} {k}"


@pytest.mark.parametrize("S", [1024, 4096])
def test_rays_training_views_second_call_and_stream(cuda0, S):
    """Views of 4 097 and 50 176 rows (224 x 224), 16 images, both sets: device against host; a second call; a caller's
    stream."""
    rng = np.random.default_rng(S)
    front = ar.ray_bank(rng, [rng.uniform(-1, 1, (4097, 2)).astype(f32), rng.uniform(-1, 1, (50176, 2)).astype(f32), np.zeros((0, 2), f32)])
    back = ar.ray_bank(rng, [rng.uniform(-0.6, 0.6, (50176, 2)).astype(f32), rng.uniform(-1, 1, (4097, 2)).astype(f32), rng.uniform(-1, 1, (3, 2)).astype(f32)])
    ids = np.array([0, 1, 2, 1, 0, 1, 1, 0, 2, 1, 0, 1, 0, 1, 1, 0])
    rot, t = augment.ray_transform(rng.integers(0, 360, 16), rng.uniform(0.5, 1.0, 16), rng.integers(-50, 50, (16, 2)), 224)
    rot[1], t[1] = (1, 0, 0, 1), (0, 0)                                                # the 50 176-row back view untouched: no filter, m = n
    want = ops.augment_rays_host(front, ids, rot, t, S, 77, back=back)
    assert int(want[1].count[1]) == S and (want[0].count > 0).sum() >= 10
    f, b = dev_bank(cuda0, front), dev_bank(cuda0, back)
    first = ops.augment_rays(f, ids, rot, t, S, 77, back=b)
    second = ops.augment_rays(f, ids, rot, t, S, 77, back=b)
    stream = torch.cuda.Stream(device=cuda0)
    stream.wait_stream(torch.cuda.current_stream(cuda0))
    with torch.cuda.stream(stream):
        third = ops.augment_rays(f, ids, rot, t, S, 77, back=b)
    stream.synchronize()
    for got in (first, second, third):
        check_rays(got[0], want[0], "front")
        check_rays(got[1], want[1], "back")


# ---------------------------------------------------------------- refusals
def test_refusals(cuda0):
    rng = np.random.default_rng(0)
    rgb, mask, _, _ = ar.image_inputs(rng, 1, 4, 4)
    d = dev_images(cuda0, dict(rgb=rgb, mask=mask))
    I = ar.rotation(4, 4, 0, 1.0)[None]
    for kw in (dict(M=np.zeros((1, 2, 3))), dict(M=I, std=(1, 0, 1)), dict(M=I, border=[[256, 1]]), dict(M=I, rect=[[0, 0, -1, 2]]),
               dict(M=I, tra1=[[0, -(2 ** 24) - 1]])):
        with pytest.raises(_capi.IsrError):
            ops.augment_images(d["rgb"], d["mask"], **kw)
    bank = dev_bank(cuda0, ar.ray_bank(rng, [rng.uniform(-1, 1, (4, 2)).astype(f32)]))
    ident, zero = np.array([[1, 0, 0, 1]], f32), np.zeros((1, 2), f32)
    L = _capi.lib()
    out = ops.augment_rays(bank, [0], ident, zero, 8, 0)
    for S in (0, 4097):
        with pytest.raises(ValueError):
            ops.augment_rays(bank, [0], ident, zero, S, 0)
        rc = L.isr_augment_rays(bank[0].data_ptr(), bank[1].data_ptr(), ops._hp(bank[2]), None, None, None, 1, ops._hp(np.zeros(1, np.int32)),
                                ops._hp(ident), ops._hp(zero), 1, S, 0, out.xys.data_ptr(), out.pos.data_ptr(), out.index.data_ptr(),
                                out.count.data_ptr(), None, None, None, None, None)
        assert rc != 0 and b"4096" in L.isr_last_error()
    n = (1 << 20) + 1
    big = (torch.zeros((n, 2), device=cuda0), torch.zeros((n, 3), device=cuda0), np.array([0, n]))
    with pytest.raises(_capi.IsrError, match="2\\^20"):
        ops.augment_rays(big, [0], ident, zero, 4, 0)
    # a back set with a pointer missing
    rc = L.isr_augment_rays(bank[0].data_ptr(), bank[1].data_ptr(), ops._hp(bank[2]), bank[0].data_ptr(), None, ops._hp(bank[2]), 1,
                            ops._hp(np.zeros(1, np.int32)), ops._hp(ident), ops._hp(zero), 1, 8, 0, out.xys.data_ptr(), out.pos.data_ptr(),
                            out.index.data_ptr(), out.count.data_ptr(), None, None, None, None, None)
    assert rc != 0 and b"back set" in L.isr_last_error()


# ---------------------------------------------------------------- PoseBatches
V, H, S, BATCH = 6, 16, 64, 2


def views(dev):
    rng = np.random.default_rng(31)
    images = torch.from_numpy(rng.uniform(0, 1, (V, H, H, 3)).astype(f32)).to(dev)
    sil = np.zeros((V, H, H), f32)
    sil[:, 3:13, 2:14] = 1
    vs = []
    for v in range(V):
        n1, n2 = 300 + 17 * v, 200 + 5 * v
        vs.append({"xys": torch.from_numpy(rng.uniform(-0.6, 0.6, (1, n1, 2)).astype(f32)), "pos_vec": torch.from_numpy(rng.uniform(-1, 1, (1, n1, 3)).astype(f32)),
                   "pos_vec_back": torch.from_numpy(rng.uniform(-1, 1, (1, n2, 3)).astype(f32)), "xys_back": torch.from_numpy(rng.uniform(-0.6, 0.6, (1, n2, 2)).astype(f32))})
    canvases = torch.from_numpy(rng.uniform(0, 1, (3, H, H, 3)).astype(f32)).to(dev)
    return images, torch.from_numpy(sil).to(dev), augment.CorrespondenceBank.from_views(vs, dev), canvases


def batches(dev, seed=4):
    images, sil, bank, canvases = views(dev)
    return augment.PoseBatches(images, sil, bank, batch_size=BATCH, sample_size=S, seed=seed, canvases=canvases, scaleFac=0.9, transScale=0.3,
                               maskMax=20, borderADD=True)


def flat(batch):
    rgb, mask, pos, xys, ex = batch
    return [rgb, mask, pos, xys, ex["mask_out"], ex["pos_points_back"], ex["xys_back"], ex["index"], ex["index_back"], ex["count"], ex["count_back"],
            ex["short"], ex["view_ids"], ex["params"].M, ex["params"].rect]


def test_pose_batches_repeat_byte_for_byte(cuda0):
    loader = batches(cuda0)
    a, b = [flat(x) for x in loader], [flat(x) for x in loader]
    assert len(a) == len(loader) == V // BATCH
    for x, y in zip(a, b):
        assert poison.same_bits(poison.to_host(x), poison.to_host(y))
    other = [flat(x) for x in batches(cuda0, seed=5)]
    assert not poison.same_bits(poison.to_host(a), poison.to_host(other))
    seen = torch.cat([x[12] for x in a]).cpu().tolist()
    assert len(set(seen)) == len(seen) == (V // BATCH) * BATCH                        # shuffled views, none twice, the short batch dropped
    for rgb, mask, pos, xys, mask_out, *_rest in a:
        assert rgb.shape == (BATCH, H, H, 3) and mask.shape == (BATCH, H, H) and pos.shape == (BATCH, S, 3) and xys.shape == (BATCH, S, 2)
        assert set(mask.unique().tolist()) <= {0.0, 1.0} and mask.sum() > 0 and torch.isfinite(rgb).all()
    # the batch is what the two ops give for its parameters: the first batch against the host build
    rgb, mask, pos, xys, ex = next(iter(loader))
    p, ids = ex["params"], ex["view_ids"].cpu().numpy()
    front = ops.augment_rays_host((loader.bank.xys.cpu().numpy(), loader.bank.pos.cpu().numpy(), loader.bank.offsets), ids, p.ray_rot.numpy(),
                                  p.ray_t.numpy(), S, 0)
    assert same(ex["count"], front.count) and not bool(ex["short"])
    inside = (xys.abs() < 1).all()
    assert bool(inside)


def test_pose_batches_feed_three_training_steps(cuda0):
    """Three pose_train_step's on 16 x 16 images with S = 64, the 3 x 3 convolution encoder and the small SIREN of
    tests/test_gpu_pose_step.py: finite losses, byte-equal on a rerun."""
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        encoder = torch.nn.Conv2d(3, 13, 3, padding=1).to(cuda0)
        field = TrainableKeyField.siren(hidden=32, hidden_layers=1, out=12, seed=0, device=cuda0)
        opt = torch.optim.Adam([{"params": field.parameters(), "lr": 3e-5}, {"params": encoder.parameters(), "lr": 3e-4}])
        gen = torch.Generator(device=cuda0).manual_seed(9)
        neg = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (1, BATCH * S, 3)).astype(f32)).to(cuda0)
        hist = []
        for rgb, mask, pos, xys, ex in batches(cuda0):
            out = pose_train_step(encoder, field, opt, rgb, mask, pos, xys, neg, generator=gen)
            hist.append(torch.stack([out["loss"], out["feature_loss"], out["mask_loss"]]))
        assert len(hist) == 3
        runs.append(torch.stack(hist).cpu().numpy())
    print("loss, feature loss and mask loss over three steps:", runs[0].tolist())
    assert np.isfinite(runs[0]).all()
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
