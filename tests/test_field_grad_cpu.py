"""CPU: the key field's backward as host code (csrc/field_grad.hpp through isr_field_backward_host / isr_field_cos_host) against
the NumPy restatement of include/isr_field_grad.h (tests/field_grad_ref.py), bit for bit: every field of the restatement's
table, N below, at and above the tile and the chain, every upstream case, a NaN point; against torch autograd in f64 inside
4 x torch-f32's own deviation; cos32 against the f64 cosine; refusals through the C ABI without a device; the ctypes table
against the header."""
import ctypes
import re

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import KeyField
from tests import field_grad_ref as fg
from tests.field_grad_ref import ROOT, f32, f64, same

vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

# the largest error of cos32 against the f64 cosine, in f32 ulp of the true value, measured by the two tests below (and by
# tools/field_grad_host_check.cpp) and rounded up to the next 0.01; sin32's is 0.5
COS32_ULP_WIDE = 0.51        # over [-2^17, 2^17]
COS32_ULP_DENSE = 0.51       # a dense grid in [-110, 110]


@pytest.fixture(scope="module")
def chain(hip_lib):
    geo = ops.field_grad_geometry()
    assert geo["chain"] == 64 and geo["chain"] % geo["tile"] == 0 and geo["slab"] % geo["chain"] == 0
    return geo["chain"]


def _host(fld, pts, dout):
    widths, omegas, Ws, bs = fld
    return ops.field_backward_host(KeyField(Ws, bs, omegas, None).pack_host, widths, pts, dout)


def _check(fld, N, chain, upstream="random"):
    widths, omegas, Ws, bs = fld
    pts, dout = fg.inputs(widths, N, upstream)
    got, want = _host(fld, pts, dout), fg.backward(Ws, bs, omegas, pts, dout, chain)
    assert same(got[0], want[0]) and same(got[1], want[1]), (widths, N, upstream)
    return got


@pytest.mark.parametrize("name", list(fg.FIELDS))
def test_host_equals_the_restatement_over_fields(chain, name):
    fld = fg.field(name)
    got = _check(fld, 2 * chain + 1, chain)
    assert np.abs(got[0]).max() > 0 and np.isfinite(got[0]).all()


def test_host_equals_the_restatement_over_N(chain):
    for name in ("3-40-33-5", "linear hidden"):
        fld = fg.field(name, seed=1)
        for N in (1, 63, 64, 65, chain - 1, chain, chain + 1, 2 * chain + 1):
            _check(fld, N, chain)
        got = _check(fld, 0, chain)
        assert got[0].size == ops.field_param_sizes(fld[0])[0] and not got[0].any() and not got[1].any()


@pytest.mark.parametrize("upstream", fg.UPSTREAMS)
def test_upstream_cases(chain, upstream):
    for name in ("3-32-12", "narrow second"):
        got = _check(fg.field(name, seed=2), chain + 7, chain, upstream)
        assert upstream != "zero" or (not got[0].any() and not got[1].any())


def test_a_nan_point_in_the_middle(chain):
    widths, omegas, Ws, bs = fld = fg.field("3-40-33-5", seed=3)
    pts, dout = fg.inputs(widths, 2 * chain + 1)
    pts[chain + 5, 2] = np.nan
    got, want = _host(fld, pts, dout), fg.backward(Ws, bs, omegas, pts, dout, chain)
    assert np.isnan(got[0]).any() and np.isnan(got[1]).any()
    assert same(got[0], want[0]) and same(got[1], want[1])            # NaNs in the restatement's places, every other entry equal


@pytest.mark.parametrize("name", list(fg.FIELDS))
def test_within_the_margin_of_torch_f64(chain, name):
    """4096 points, the issue's measurement: every dW_l and db_l within 4 x torch-f32's own largest deviation from torch-f64
    on that array.  The multiples go to profiles/field_grad_parity.json when ISR_RECORD_PARITY is set."""
    widths, omegas, Ws, bs = fld = fg.field(name, seed=4)
    pts, dout = fg.inputs(widths, 4096, seed=4)
    r32 = fg.torch_grads(Ws, bs, omegas, pts, dout, torch.float32)
    r64 = fg.torch_grads(Ws, bs, omegas, pts, dout, torch.float64)
    assert fg.within_margin(f"{name} N 4096", widths, _host(fld, pts, dout), r32, r64, "host")


def _cos_error(a):
    a = a.astype(f32)
    got = ops.field_cos_host(a).astype(f64)
    ref = np.cos(a.astype(f64))
    err = np.abs(got - ref) / np.spacing(np.abs(ref).astype(f32)).astype(f64)
    assert np.all(np.abs(got) <= 1.0)
    assert same(ops.field_cos_host(a), fg.sincos32(a)[1])                      # the restatement's cosine is the library's
    return float(err.max()), float(a[np.argmax(err)])


def test_cos32_over_the_wide_range(hip_lib):
    rng = np.random.default_rng(0)
    lim, n = 2.0 ** 17, 600_000
    logs = np.exp(rng.uniform(np.log(1e-38), np.log(lim), n)) * rng.choice([-1.0, 1.0], n)
    halfpi = np.arange(-83443, 83444) * (np.pi / 2)                             # every multiple of pi/2 inside the range
    a = np.concatenate([rng.uniform(-lim, lim, n), np.linspace(-lim, lim, 100_001), logs, halfpi, [0.0, lim, -lim, 1e-45, -1e-45]])
    a = a[np.abs(a) <= lim]
    worst, at = _cos_error(a)
    print(f"cos32 over [-2^17, 2^17]: {a.size} arguments, largest error {worst:.4f} ulp at {at!r}")
    assert worst <= COS32_ULP_WIDE


def test_cos32_over_the_dense_grid(hip_lib):
    worst, at = _cos_error(np.linspace(-110.0, 110.0, 4_000_001))
    print(f"cos32 over [-110, 110]: 4000001 arguments, largest error {worst:.4f} ulp at {at!r}")
    assert worst <= COS32_ULP_DENSE


def test_cos32_special_values(hip_lib):
    one = ops.field_cos_host(np.array([0.0, -0.0], f32))
    assert one[0] == 1 and one[1] == 1
    assert np.isnan(ops.field_cos_host(np.array([np.nan, np.inf, -np.inf], f32))).all()
    far = np.array([2.0 ** 18, -2.0 ** 40, 3e38, -3.4e38], f32)
    assert np.all(np.abs(ops.field_cos_host(far)) <= 1.0)


def test_refusals_without_a_device(hip_lib):
    L = hip_lib
    w = np.array([3, 64, 12], np.int32)
    nb, nbt = L.isr_field_pack_bytes(2, vp(w)), L.isr_field_grad_pack_bytes(2, vp(w))
    assert nbt > 0 and nbt % 4 == 0 and L.isr_field_grad_workspace_bytes(2, vp(w), 100) > 0
    assert L.isr_field_grad_workspace_bytes(2, vp(w), 10 ** 6) == L.isr_field_grad_workspace_bytes(2, vp(w), L.isr_field_grad_geometry(2))     # bounded by the slab
    assert L.isr_field_grad_workspace_bytes(2, vp(w), 65) > L.isr_field_grad_workspace_bytes(2, vp(w), 64)
    bad = [(0, w), (9, np.array([3] + [8] * 9, np.int32)), (2, np.array([4, 64, 12], np.int32)), (2, np.array([3, 257, 12], np.int32)),
           (2, np.array([3, 64, 33], np.int32)), (2, np.array([3, 0, 12], np.int32))]
    for n, ww in bad:
        assert L.isr_field_grad_pack_bytes(n, vp(ww)) == 0 and L.isr_last_error()
        assert L.isr_field_grad_workspace_bytes(n, vp(ww), 64) == 0 and L.isr_last_error()
    assert L.isr_field_grad_pack_bytes(2, None) == 0 and L.isr_field_grad_workspace_bytes(2, None, 64) == 0
    assert L.isr_field_grad_workspace_bytes(2, vp(w), -1) == 0
    assert L.isr_field_grad_geometry(4) == -1 and L.isr_field_grad_geometry(-1) == -1
    pack, packT = np.zeros(nb // 4, f32), np.zeros(nbt // 4, f32)
    pts, dout = np.zeros((4, 3), f32), np.zeros((4, 12), f32)
    dW, db = np.zeros(64 * 3 + 12 * 64, f32), np.zeros(76, f32)
    om, sn = np.ones(2, f32), np.ones(2, np.int32)
    host = lambda *a: L.isr_field_backward_host(*a)
    assert host(vp(pack), nb, 2, vp(w), vp(pts), 4, vp(dout), 12, vp(dW), vp(db)) == 0
    assert host(None, nb, 2, vp(w), vp(pts), 4, vp(dout), 12, vp(dW), vp(db)) == -1 and b"null" in L.isr_last_error()
    assert host(vp(pack), nb, 2, None, vp(pts), 4, vp(dout), 12, vp(dW), vp(db)) == -1
    assert host(vp(pack), nb, 2, vp(w), None, 4, vp(dout), 12, vp(dW), vp(db)) == -1
    assert host(vp(pack), nb, 2, vp(w), vp(pts), 4, None, 12, vp(dW), vp(db)) == -1
    assert host(vp(pack), nb, 2, vp(w), vp(pts), 4, vp(dout), 11, vp(dW), vp(db)) == -1 and b"ld_dout" in L.isr_last_error()
    assert host(vp(pack), nb - 4, 2, vp(w), vp(pts), 4, vp(dout), 12, vp(dW), vp(db)) == -1 and b"pack_bytes" in L.isr_last_error()
    assert host(vp(pack), nb, 2, vp(w), vp(pts), -1, vp(dout), 12, vp(dW), vp(db)) == -1
    assert host(vp(pack), nb, 2, vp(np.array([3, 300, 12], np.int32)), vp(pts), 4, vp(dout), 12, vp(dW), vp(db)) == -1
    # the device entries refuse before any device is touched (the pointers here are host arrays: never dereferenced)
    ws_bytes = L.isr_field_grad_workspace_bytes(2, vp(w), 4)
    ws = np.zeros(8, f32)
    dev = lambda **kw: L.isr_field_backward(*[kw.get(k, v) for k, v in (
        ("pack", vp(pack)), ("pack_bytes", nb), ("packT", vp(packT)), ("packT_bytes", nbt), ("n_layers", 2), ("widths", vp(w)), ("pts", vp(pts)),
        ("N", 4), ("dout", vp(dout)), ("ld_dout", 12), ("dW", vp(dW)), ("db", vp(db)), ("ws", vp(ws)), ("ws_bytes", ws_bytes), ("stream", None))])
    for kw, text in (({"pack": None}, b"null"), ({"packT": None}, b"null"), ({"widths": None}, b"null"), ({"pts": None}, b"null"),
                     ({"dout": None}, b"null"), ({"ws": None}, b"null"), ({"ws_bytes": ws_bytes - 256}, b"ws_bytes"),
                     ({"ws_bytes": 0}, b"ws_bytes"), ({"ld_dout": 11}, b"ld_dout"), ({"packT_bytes": nbt - 4}, b"packT_bytes"),
                     ({"pack_bytes": nb + 4}, b"pack_bytes"), ({"N": -1}, b"N"), ({"n_layers": 0}, b"layers"),
                     ({"widths": vp(np.array([3, 64, 40], np.int32))}, b"widths")):
        assert dev(**kw) == -1 and text in L.isr_last_error(), kw
    packd = lambda **kw: L.isr_field_pack_device(*[kw.get(k, v) for k, v in (
        ("n_layers", 2), ("widths", vp(w)), ("W", vp(dW)), ("b", vp(db)), ("omega", vp(om)), ("sine", vp(sn)), ("pack", vp(pack)),
        ("pack_bytes", nb), ("packT", vp(packT)), ("packT_bytes", nbt), ("stream", None))])
    for kw in ({"W": None}, {"b": None}, {"omega": None}, {"sine": None}, {"pack": None}, {"packT": None}, {"pack_bytes": nb - 4},
               {"packT_bytes": nbt + 4}, {"widths": vp(np.array([3, 300, 12], np.int32))}):
        assert packd(**kw) == -1 and L.isr_last_error(), kw
    assert L.isr_field_cos_host(None, 3, vp(ws)) == -1 and L.isr_field_cos_host(None, 0, None) == 0


def test_wrappers_refuse_host_tensors(hip_lib):
    with pytest.raises(_capi.IsrError):
        ops.field_backward(torch.zeros(8), torch.zeros(8), (3, 12), torch.zeros(4, 3), torch.zeros(4, 12))
    with pytest.raises(_capi.IsrError):
        ops.field_pack_device((3, 12), torch.zeros(36), torch.zeros(12), (30.0,))


def test_ctypes_table_matches_the_header(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_field_grad.h").read_text(), flags=re.S)
    decls = dict(re.findall(r"\b(isr_[a-z0-9_]+)\s*\(([^)]*)\)", text))
    assert sorted(decls) == sorted(_capi.FIELD_GRAD_SIGNATURES) and len(decls) == 7
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_field_grad.h but not exported"
        assert len(_capi.FIELD_GRAD_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name


def test_trainable_key_field_builds_without_a_device(hip_lib):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import TrainableKeyField
    field = TrainableKeyField.siren(hidden=40, hidden_layers=1, out=5, seed=1)
    assert field.widths == (3, 40, 40, 5) and field.omegas == (30.0, 30.0, 30.0)
    assert sorted(field.state_dict()) == sorted([f"weights.{l}" for l in range(3)] + [f"biases.{l}" for l in range(3)])
    assert all(p.requires_grad for p in field.parameters())
    assert float(field.weights[0].detach().abs().max()) <= 1 / 3 and float(field.weights[1].detach().abs().max()) <= (6 / 40) ** 0.5 / 30
    assert TrainableKeyField.siren(hidden=8, hidden_layers=0, out=4, outermost_linear=True).omegas == (30.0, None)
    frozen = field.to_key_field()                                              # host-only while the parameters are on the CPU
    again = TrainableKeyField.from_key_field(frozen, device="cpu")             # the pack read back: narrow and matrix-core layers
    assert all(torch.equal(a, b) for a, b in zip(field.parameters(), again.parameters()))
    lin = [torch.nn.Linear(3, 8), torch.nn.Linear(8, 4)]
    copy = TrainableKeyField.from_linears(lin, (30.0, None))
    assert copy.widths == (3, 8, 4) and torch.equal(copy.weights[1], lin[1].weight) and copy.weights[1] is not lin[1].weight
    with pytest.raises(_capi.IsrError):
        TrainableKeyField([torch.zeros(300, 3)], [torch.zeros(300)], (30.0,))
    with pytest.raises(ValueError):
        TrainableKeyField([torch.zeros(8, 3), torch.zeros(4, 9)], [torch.zeros(8), torch.zeros(4)], (30.0, 30.0))
    with pytest.raises(ValueError):
        TrainableKeyField.from_linears([torch.nn.Linear(3, 8, bias=False)], (30.0,))
    with pytest.raises(_capi.IsrError):
        field(torch.zeros(4, 3))                                               # CPU tensors: there is no CPU fallback
    with pytest.raises(NotImplementedError):
        field(torch.zeros(4, 3, requires_grad=True))
