"""GPU: the key field's backward (isr_field_backward) against the host build of the same header (which
tests/test_field_grad_cpu.py holds to the NumPy restatement of include/isr_field_grad.h), bit for bit with NaN-aware equality,
for dW and db: every field of tests/field_grad_ref.py at N below, at and above the tile and the chain (64) and the slab;
forced slab sizes; the device-side packing against the host pack; the contracts (poisoned outputs, packs and workspace, a
reused workspace, a caller's stream, a wider upstream, gradients left out); then TrainableKeyField under autograd: forward bits,
.grad against the entry, the margin against torch in f64 on the device, an optimizer step, and trainPose.py's step end to end."""
import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import losses, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import IsrError
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import KeyField, TrainableKeyField
from tests import contrastive_ref as cr
from tests import field_grad_ref as fg
from tests import poison
from tests.field_grad_ref import f32, same

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _flat(arrays, dev):
    return _t(np.concatenate([np.asarray(a, f32).reshape(-1) for a in arrays]), dev)


def _packs(dev, widths, omegas, Ws, bs):
    return ops.field_pack_device(widths, _flat(Ws, dev), _flat(bs, dev), omegas)


def _device(dev, fld, pts, dout, **kw):
    widths, omegas, Ws, bs = fld
    pack, packT = _packs(dev, widths, omegas, Ws, bs)
    dW, db = ops.field_backward(pack, packT, widths, _t(pts, dev), _t(dout, dev), **kw)
    return tuple(None if x is None else x.cpu().numpy() for x in (dW, db))


def _host(fld, pts, dout):
    widths, omegas, Ws, bs = fld
    return ops.field_backward_host(KeyField(Ws, bs, omegas, None).pack_host, widths, pts, dout)


def _check(dev, fld, N, upstream="random", **kw):
    pts, dout = fg.inputs(fld[0], N, upstream)
    got, want = _device(dev, fld, pts, dout, **kw), _host(fld, pts, dout)
    for name, a, b in zip(("dW", "db"), got, want):
        assert same(a, b), (name, fld[0], N, upstream, kw)
    return got


@pytest.mark.parametrize("name", list(fg.FIELDS))
def test_device_equals_host(cuda0, name):
    geo = ops.field_grad_geometry()
    assert geo == {"chain": 64, "tile": 64, "slab": 16384, "batch": 8192}                      # the widths the sizes here straddle
    fld = fg.field(name)
    for N in (0, 1, 63, 64, 65, 129, 255, 256, 257, 513):
        got = _check(cuda0, fld, N)
        assert N or (not got[0].any() and not got[1].any())


@pytest.mark.parametrize("name", ["3-40-33-5", "narrow second"])
def test_one_more_than_a_batch_and_than_a_slab(cuda0, name):
    geo = ops.field_grad_geometry()
    for N in (geo["batch"] + 1, geo["slab"] + 1):
        _check(cuda0, fg.field(name), N)


@pytest.mark.parametrize("name", ["3-40-33-5", "3-256-256-256-12", "linear hidden"])
def test_4097_points_and_forced_slabs(cuda0, name):
    """A ragged last tile and a ragged last chain; the same N through slabs of one chain, of sixteen and of the default."""
    fld = fg.field(name)
    base = _check(cuda0, fld, 4097)
    for slab in (64, 1024):
        got = _check(cuda0, fld, 4097, slab=slab)
        assert same(got[0], base[0]) and same(got[1], base[1])


@pytest.mark.parametrize("upstream", fg.UPSTREAMS)
def test_upstream_cases(cuda0, upstream):
    for name in ("3-40-33-5", "linear hidden", "narrow second"):
        got = _check(cuda0, fg.field(name), 321, upstream)
        assert upstream != "zero" or (not got[0].any() and not got[1].any())


def test_a_nan_point_in_the_middle(cuda0):
    for name in ("3-40-33-5", "3-256-256-256-12"):
        fld = fg.field(name)
        pts, dout = fg.inputs(fld[0], 300)
        pts[150, 1] = np.nan
        got, want = _device(cuda0, fld, pts, dout), _host(fld, pts, dout)
        assert same(got[0], want[0]) and same(got[1], want[1]) and np.isnan(got[0]).any()


@pytest.mark.parametrize("name", list(fg.FIELDS))
def test_device_pack_is_the_host_pack_and_evaluates_alike(cuda0, name):
    widths, omegas, Ws, bs = fg.field(name, seed=3)
    kf = KeyField(Ws, bs, omegas, cuda0)
    pack, packT = _packs(cuda0, widths, omegas, Ws, bs)
    assert np.array_equal(pack.cpu().numpy().view(np.uint32), kf.pack_host.view(np.uint32))
    assert np.array_equal(packT.cpu().numpy().view(np.uint32), fg.pack_t(widths, Ws).view(np.uint32))
    pts = _t(fg.inputs(widths, 130)[0], cuda0)
    assert torch.equal(ops.field_eval(pack, widths, pts).view(torch.int32), kf(pts).view(torch.int32))


def test_every_byte_of_every_output_is_written(cuda0, monkeypatch):
    for name, N in (("3-40-33-5", 321), ("3-256-256-256-12", 70), ("narrow second", 16385), ("3-12", 0)):
        widths, omegas, Ws, bs = fld = fg.field(name)
        pts, dout = fg.inputs(widths, N)

        def call():
            pack, packT = _packs(cuda0, widths, omegas, Ws, bs)                # both packs, dW, db and the workspace: torch.empty
            return (pack, packT, *ops.field_backward(pack, packT, widths, _t(pts, cuda0), _t(dout, cuda0)))

        a, b = poison.run_twice(monkeypatch, call)
        assert poison.same_bits(a, b)
        want = _host(fld, pts, dout)
        assert same(a[2].numpy(), want[0]) and same(a[3].numpy(), want[1])


def test_second_call_a_reused_workspace_and_a_callers_stream(cuda0):
    fld = fg.field("3-40-33-5")
    pts, dout = fg.inputs(fld[0], 16385)                                       # one more than a slab
    want = _host(fld, pts, dout)
    ops.clear_workspaces()
    for _ in range(2):
        got = _device(cuda0, fld, pts, dout)
        assert same(got[0], want[0]) and same(got[1], want[1])
    small = fg.inputs(fld[0], 65)                                               # the large call's leftovers in the workspace
    got, w65 = _device(cuda0, fld, *small), _host(fld, *small)
    assert same(got[0], w65[0]) and same(got[1], w65[1])
    side = torch.cuda.Stream(cuda0)
    side.wait_stream(torch.cuda.current_stream(cuda0))
    with torch.cuda.stream(side):
        got = _device(cuda0, fld, pts, dout)
    side.synchronize()
    assert same(got[0], want[0]) and same(got[1], want[1])


def test_a_wider_upstream_with_garbage_in_the_extra_column(cuda0):
    fld = fg.field("3-40-33-5")
    pts, dout = fg.inputs(fld[0], 321)
    wide = np.concatenate([dout, np.full((321, 1), np.nan, f32)], axis=1)
    wide[::2, -1] = 3e38
    got, want = _device(cuda0, fld, pts, wide), _host(fld, pts, dout)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert same(_host(fld, pts, wide)[0], want[0])


def test_each_gradient_left_out_in_turn(cuda0):
    fld = fg.field("3-40-33-5")
    pts, dout = fg.inputs(fld[0], 321)
    full = _device(cuda0, fld, pts, dout)
    for need in ((True, False), (False, True), (False, False)):
        got = _device(cuda0, fld, pts, dout, need=need)
        for i in range(2):
            assert same(got[i], full[i]) if need[i] else got[i] is None


def test_refusals_on_the_device(cuda0):
    widths, omegas, Ws, bs = fg.field("3-12")
    pack, packT = _packs(cuda0, widths, omegas, Ws, bs)
    pts, dout = (_t(x, cuda0) for x in fg.inputs(widths, 5))
    with pytest.raises(IsrError):
        ops.field_backward(pack, packT, widths, pts.cpu(), dout)
    with pytest.raises(IsrError):
        ops.field_pack_device(widths, _flat(Ws, "cpu"), _flat(bs, cuda0), omegas)
    with pytest.raises(ValueError):
        ops.field_backward(pack, packT, widths, pts, dout[:, :11].contiguous())
    with pytest.raises(IsrError):
        ops.field_backward(pack, packT[:-1], widths, pts, dout)


# ---- autograd

def _trainable(dev, name, seed=0):
    widths, omegas, Ws, bs = fg.field(name, seed)
    return TrainableKeyField(Ws, bs, omegas, dev), (widths, omegas, Ws, bs)


def _grads(field):
    return (torch.cat([w.grad.reshape(-1) for w in field.weights]).cpu().numpy(),
            torch.cat([b.grad.reshape(-1) for b in field.biases]).cpu().numpy())


@pytest.mark.parametrize("name", ["3-40-33-5", "3-256-256-256-12", "linear hidden"])
def test_forward_is_keyfield_and_grad_is_the_entry(cuda0, name):
    field, (widths, omegas, Ws, bs) = _trainable(cuda0, name)
    kf = KeyField(Ws, bs, omegas, cuda0)
    pts = _t(fg.inputs(widths, 321)[0], cuda0).reshape(3, 107, 3)
    out = field(pts)
    assert out.requires_grad and out.shape == (3, 107, widths[-1])
    assert torch.equal(out.detach().view(torch.int32), kf(pts).view(torch.int32))
    with torch.no_grad():
        assert not field(pts).requires_grad
    wide = field.batched_customForward(pts)
    assert torch.equal(wide.detach().view(torch.int32), kf.batched_customForward(pts).view(torch.int32))
    pack, packT = _packs(cuda0, widths, omegas, Ws, bs)
    rows = pts.reshape(-1, 3)
    out.sum().backward()
    want = ops.field_backward(pack, packT, widths, rows, torch.ones((321, widths[-1]), device=cuda0))
    assert all(same(a, b.cpu().numpy()) for a, b in zip(_grads(field), want))
    field.zero_grad(set_to_none=True)
    leaf = wide.detach().requires_grad_(True)
    (3 * torch.tanh(leaf).square().sum()).backward()
    (3 * torch.tanh(wide).square().sum()).backward()
    want = ops.field_backward(pack, packT, widths, rows, leaf.grad.reshape(321, -1).contiguous())
    assert all(same(a, b.cpu().numpy()) for a, b in zip(_grads(field), want))


def test_needs_input_grad_is_honoured(cuda0):
    field, (widths, *_rest) = _trainable(cuda0, "3-40-33-5")
    pts = _t(fg.inputs(widths, 70)[0], cuda0)
    field(pts).sum().backward()
    full = [p.grad.clone() for p in field.parameters()]
    field.zero_grad(set_to_none=True)
    field.weights[1].requires_grad_(False)
    for b in field.biases:
        b.requires_grad_(False)
    field(pts).sum().backward()
    for p, g in zip(field.parameters(), full):
        assert (p.grad is None) if not p.requires_grad else torch.equal(p.grad.view(torch.int32), g.view(torch.int32))


@pytest.mark.parametrize("name", ["3-40-33-5", "3-256-256-256-12", "linear hidden"])
def test_gradients_within_the_margin_of_torch_f64_on_the_device(cuda0, name):
    field, (widths, omegas, Ws, bs) = _trainable(cuda0, name, seed=5)
    pts, dout = fg.inputs(widths, 4096, seed=5)
    (field(_t(pts, cuda0)) * _t(dout, cuda0)).sum().backward()
    r32 = fg.torch_grads(Ws, bs, omegas, pts, dout, torch.float32, cuda0, chunks=16)
    r64 = fg.torch_grads(Ws, bs, omegas, pts, dout, torch.float64, cuda0, chunks=16)
    assert fg.within_margin(f"{name} N 4096", widths, _grads(field), r32, r64, "device")


def test_an_optimizer_step_repacks(cuda0):
    field, (widths, omegas, *_rest) = _trainable(cuda0, "3-40-33-5")
    pts = _t(fg.inputs(widths, 130)[0], cuda0)
    opt = torch.optim.Adam(field.parameters(), lr=1e-3)
    with torch.no_grad():
        before = field(pts).clone()
    field(pts).square().sum().backward()
    opt.step()
    with torch.no_grad():
        after = field(pts)                                                      # no gradients: repacked because the versions moved
    Ws = [w.detach().cpu().numpy() for w in field.weights]
    kf = field.to_key_field()
    assert not torch.equal(after, before)
    assert torch.equal(after.view(torch.int32), kf(pts).view(torch.int32))
    pack, packT = field._packs()
    assert np.array_equal(pack.cpu().numpy().view(np.uint32), kf.pack_host.view(np.uint32))          # the padding is still zero
    assert np.array_equal(packT.cpu().numpy().view(np.uint32), fg.pack_t(widths, Ws).view(np.uint32))
    again = TrainableKeyField.from_key_field(kf)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again.parameters(), field.parameters()))


def test_the_training_step_end_to_end(cuda0):
    """trainPose.py's step without the UNet at B = 2, S = 64, M = 64, D = 12: keys and negatives from batched_customForward,
    returnCrossEntropyWithNeg, backward; the parameter gradients against the same chain in torch f64; five Adam steps."""
    B, S, M = 2, 64, 64
    field = TrainableKeyField.siren(hidden=256, hidden_layers=2, out=12, seed=11, device=cuda0)
    assert field.widths == (3, 256, 256, 256, 12)
    rng = np.random.default_rng(12)
    kp, npt = rng.uniform(-1, 1, (B, S, 3)).astype(f32), rng.uniform(-1, 1, (B, M, 3)).astype(f32)
    q = (rng.standard_normal((B, S, 13)) * 3).astype(f32)
    q[..., -1] = 0

    def chain(dtype):
        Ws, bs = [w.detach().cpu().numpy() for w in field.weights], [b.detach().cpu().numpy() for b in field.biases]
        tf = fg.field_ref.TorchField(Ws, bs, field.omegas).to(device=cuda0, dtype=dtype)

        def keys(x):
            x = _t(x, cuda0).to(dtype)
            for m, om in zip(tf.linears, tf.omegas):
                x = torch.sin(om * m(x)) if om is not None else m(x)
            return torch.cat([x, torch.zeros_like(x[..., :1])], dim=-1)

        cr.torch_loss(_t(q, cuda0).to(dtype), keys(kp), keys(npt)).backward()
        return [(m.weight.grad.double().cpu().numpy(), m.bias.grad.double().cpu().numpy()) for m in tf.linears]

    def loss_of():
        return losses.returnCrossEntropyWithNeg(_t(q, cuda0), field.batched_customForward(_t(kp, cuda0)),
                                                field.batched_customForward(_t(npt, cuda0)))

    loss_of().backward()
    assert fg.within_margin("training step B 2 S 64 M 64", field.widths, _grads(field), chain(torch.float32), chain(torch.float64), "device")
    opt = torch.optim.Adam(field.parameters(), lr=1e-4)
    history = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss = loss_of()
        loss.backward()
        opt.step()
        history.append(float(loss.detach()))
    print("loss over five Adam steps:", history)
    assert history[-1] < history[0]


def test_points_that_require_a_gradient_and_cpu_tensors_are_refused(cuda0):
    field, (widths, *_rest) = _trainable(cuda0, "3-12")
    pts = _t(fg.inputs(widths, 5)[0], cuda0)
    with pytest.raises(NotImplementedError):
        field(pts.clone().requires_grad_(True))
    with pytest.raises(IsrError):
        field(pts.cpu())
    with pytest.raises(IsrError):
        _trainable("cpu", "3-12")[0](pts)
