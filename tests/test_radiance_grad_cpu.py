"""The radiance field's backward without a GPU (include/isr_radiance_grad.h): the host build of csrc/radiance_grad.hpp against
the NumPy restatement of the header bit for bit, slope32 / dexp32 against f64, every gradient array of the reference's
executed code (tests/golden/ref_radiance_grad.npz) within PARITY_MARGIN x the reference's own f32 error, the refusals, and
fields.TrainableRadianceField as far as it goes on the CPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, fields, ops
from tests import density_ref as dr
from tests import radiance_grad_ref as gr
from tests import radiance_ref as rr
from tests import ref_fields as rf

ROOT = Path(__file__).resolve().parent.parent
f32, f64 = np.float32, np.float64
CHAIN = 64


def vp(a):
    return None if a is None else a.ctypes.data


def _restated(name, o, d, ln, dd, dc):
    return gr.backward(gr.host_field(name)[1], dr.frequencies(gr.FIELDS[name][0]), gr.BETA, o, d, ln, dd, dc, CHAIN)


def _both(name, N, P, kind="random"):
    o, d, ln = rr.bundle(N, P)
    dd, dc = gr.upstream(N, P, gr.FIELDS[name][3], kind)
    return gr.host_backward(name, o, d, ln, dd, dc), _restated(name, o, d, ln, dd, dc)


@pytest.mark.parametrize("name", [n for n in gr.FIELDS if n != gr.REFERENCE])
def test_host_is_the_restatement_at_every_shape(hip_lib, name):
    assert hip_lib.isr_radiance_grad_geometry(0) == CHAIN
    for N, P in gr.SHAPES:                 # N * P at 0, 1, 63, 64, 65, 129; 64 and 65 rays in a block; a ray over two blocks; ragged
        (hW, hb), (rW, rb) = _both(name, N, P)
        assert gr.same(hW, rW) and gr.same(hb, rb), (name, N, P)
        if N == 0:
            assert not hW.view(np.uint32).any() and not hb.view(np.uint32).any()


@pytest.mark.parametrize("kind", gr.UPSTREAMS)
def test_host_is_the_restatement_for_every_upstream(hip_lib, kind):
    for name in ("H4 5 Wc5 C3", "H4 32-33 Wc40 C3"):
        (hW, hb), (rW, rb) = _both(name, 5, 13, kind)
        assert gr.same(hW, rW) and gr.same(hb, rb), (name, kind)
        if kind in ("zeros", "both null"):
            assert not hW.view(np.uint32).any() and not hb.view(np.uint32).any()      # every gradient exactly +0
        else:
            assert np.abs(hW).max() > 0


def test_host_is_the_restatement_at_the_reference_widths(hip_lib):
    (hW, hb), (rW, rb) = _both(gr.REFERENCE, 3, 2)           # a handful of points
    assert gr.same(hW, rW) and gr.same(hb, rb)


def test_need_leaves_an_output_out(hip_lib):
    name = "H4 5 Wc5 C3"
    o, d, ln = rr.bundle(5, 13)
    dd, dc = gr.upstream(5, 13, 3)
    hW, hb = gr.host_backward(name, o, d, ln, dd, dc)
    assert gr.same(gr.host_backward(name, o, d, ln, dd, dc, need=(True, False))[0], hW)
    assert gr.same(gr.host_backward(name, o, d, ln, dd, dc, need=(False, True))[1], hb)


def test_a_nan_point_and_a_zero_direction(hip_lib):
    name = "H4 32-33 Wc40 C3"
    o, d, ln = rr.bundle(43, 3)                               # ray 1 has a zero direction
    assert not d[1].any()
    dd, dc = gr.upstream(43, 3, 3)
    hW, hb = gr.host_backward(name, o, d, ln, dd, dc)
    assert np.isfinite(hW).all() and np.isfinite(hb).all()
    ln = ln.copy()
    ln[20, 1] = np.nan                                        # one NaN point between clean ones
    (hW, hb), (rW, rb) = gr.host_backward(name, o, d, ln, dd, dc), _restated(name, o, d, ln, dd, dc)
    assert np.isnan(rW).any() and gr.same(hW, rW) and gr.same(hb, rb)       # NaN exactly where the restatement has it
    parts = gr.split(name, hW, hb)
    assert np.isnan(parts["db_colour2"]).all() and np.isnan(parts["dW_mlp0"]).all()


def test_slopes_within_one_ulp(hip_lib):
    """slope32 and dexp32 against their f64 values over [-110, 110] and at the beta z = 20 seam; the measured ulp is recorded."""
    z = np.concatenate([np.linspace(-110, 110, 400001), np.linspace(-11, 11, 200001), [0.0, -0.0]]).astype(f32)
    seam = np.array([2.0], f32)                               # beta z = 20 and the f32 values around it
    for _ in range(8):
        seam = np.unique(np.concatenate([seam, np.nextafter(seam, f32(4.0)), np.nextafter(seam, f32(0.0))]))
    z = np.concatenate([z, seam])
    sl, de = ops.radiance_grad_slopes_host(z, gr.BETA)
    assert gr.same(sl, gr.slope32(z, gr.BETA)) and gr.same(de, gr.dexp32(z))        # the restatement's bits
    t = f64(f32(gr.BETA)) * z.astype(f64)
    with np.errstate(over="ignore"):
        sl64 = np.where(t > 20.0, 1.0, 1.0 / (1.0 + np.exp(-t)))
        de64 = np.exp(-z.astype(f64))
    assert np.all(sl[t > 20.0] == 1.0) and np.all((sl >= 0) & (sl <= 1)) and np.all(sl[t < 16.0] < 1.0)

    def ulps(got, want):
        fin = np.isfinite(want) & (np.abs(want) < 3.4e38) & (np.abs(want) > 1.2e-38)      # f32's normal range
        u = np.spacing(np.abs(want[fin]).astype(f32)).astype(f64)
        return float((np.abs(got[fin].astype(f64) - want[fin]) / u).max())
    worst = {"slope32_ulp": ulps(sl, sl64), "dexp32_ulp": ulps(de, de64)}
    print(worst)
    gr.record("slopes", "against f64 over [-110, 110] and the seam", worst)
    assert worst["slope32_ulp"] <= 1.0 and worst["dexp32_ulp"] <= 1.0
    big = de64 >= 3.5e38
    assert np.all(np.isinf(de[big])) and np.all(de[de64 < 1e-46] == 0)
    nan = ops.radiance_grad_slopes_host(np.array([np.nan], f32), gr.BETA)
    assert np.isnan(nan[0]).all() and np.isnan(nan[1]).all()


def _fixture_field(g, tag, device=None):
    W = lambda n: g[f"{tag}_{n}.weight"]
    b = lambda n: g[f"{tag}_{n}.bias"]
    trunk, colour = ("mlp.0", "mlp.2", "density_layer.0"), ("color_layer.0", "color_layer.2")
    return fields.RadianceField([W(n) for n in trunk], [b(n) for n in trunk], [W(n) for n in colour], [b(n) for n in colour],
                                g[f"{tag}_frequencies"], 10.0, device)


@pytest.mark.parametrize("tag", ["h60", "h4", "hot"])
def test_parity_against_the_reference_fixture(hip_lib, tag):
    """Every gradient array within PARITY_MARGIN x the reference's own f32 deviation from f64.  No entry is excused."""
    g = rf.load("ref_radiance_grad")
    assert np.array_equal(rr.normalize_host(g["directions"]), g["unit_directions"])          # the library embeds the fixture's unit vectors
    fld = _fixture_field(g, tag)
    dW, db = ops.radiance_backward_host(fld.rpack_host, fld.widths, fld.H, fld.Wc, fld.C, g["origins"], g["directions"],
                                        g["lengths"], g["A"][:, :, 0], g["B"])
    ours = gr.split((fld.widths, fld.H, fld.Wc, fld.C), dW, db)
    names = {"mlp.0": "mlp0", "mlp.2": "mlp1", "density_layer.0": "density", "color_layer.0": "colour1", "color_layer.2": "colour2"}
    entry, ok = {}, True
    for ref_name, mine in names.items():
        for kind, pre in (("weight", "dW"), ("bias", "db")):
            g64, E = g[f"{tag}_g64_{ref_name}.{kind}"], float(g[f"{tag}_E_{ref_name}.{kind}"])
            assert np.isfinite(E) and E > 0
            dev = float(np.abs(ours[f"{pre}_{mine}"].astype(f64) - g64.reshape(ours[f"{pre}_{mine}"].shape)).max())
            print(f"{tag} {ref_name}.{kind}: deviation {dev:.3e}, E {E:.3e}, ratio {dev / E:.2f}")
            entry[f"{ref_name}.{kind}"] = {"deviation": dev, "E_ref": E, "ratio": dev / E}
            ok = ok and dev <= gr.PARITY_MARGIN * E
    gr.record("host vs the reference's executed code (ref_radiance_grad.npz)", tag, entry)
    assert ok, entry


def test_refusals_without_a_device(hip_lib):
    L = hip_lib
    w = np.array([32, 33], np.int32)
    shape = (2, vp(w), 4, 40, 3)
    nb, nbt = L.isr_radiance_pack_bytes(*shape), L.isr_radiance_grad_pack_bytes(*shape)
    assert nbt > 0 and nbt % 4 == 0
    wsb = lambda N, P: L.isr_radiance_grad_workspace_bytes(*shape, N, P)
    slab = L.isr_radiance_grad_geometry(2)
    assert 0 < wsb(1, 64) < wsb(1, 65) < wsb(100, 100) and wsb(10 ** 6, 16) == wsb(slab // 16 + 8, 16)      # bounded by the slab
    assert wsb(-1, 3) == 0 and wsb(4, 0) == 0 and wsb(4, 4097) == 0 and L.isr_last_error()
    for bad in ((0, vp(w), 4, 40, 3), (5, vp(np.array([8] * 5, np.int32)), 4, 40, 3), (2, vp(np.array([32, 257], np.int32)), 4, 40, 3),
                (2, vp(w), 65, 40, 3), (2, vp(w), 4, 0, 3), (2, vp(w), 4, 40, 33), (2, None, 4, 40, 3)):
        assert L.isr_radiance_grad_pack_bytes(*bad) == 0 and L.isr_last_error()
        assert L.isr_radiance_grad_workspace_bytes(*bad, 4, 4) == 0
    assert L.isr_radiance_grad_geometry(4) == -1 and L.isr_radiance_grad_geometry(-1) == -1
    assert [L.isr_radiance_grad_geometry(i) for i in range(4)] == [64, 64, slab, L.isr_radiance_grad_geometry(3)]
    pack, packT = np.zeros(nb // 4, f32), np.zeros(nbt // 4, f32)
    pack[0] = 10.0
    o, d, ln = (np.ascontiguousarray(a) for a in rr.bundle(4, 5))
    nw, nbias = ops.radiance_param_sizes((32, 33), 4, 40, 3)
    dW, db, ws = np.zeros(nw, f32), np.zeros(nbias, f32), np.zeros(8, f32)
    base = dict(pack=vp(pack), pack_bytes=nb, n_hidden=2, widths=vp(w), H=4, Wc=40, C=3, o=vp(o), d=vp(d), ln=vp(ln), N=4, P=5, dd=None,
                dc=None, dW=vp(dW), db=vp(db))
    host = lambda **kw: L.isr_radiance_backward_host(*{**base, **kw}.values())
    assert host() == 0 and not dW.any()
    for kw, text in (({"pack": None}, b"null"), ({"widths": None}, b"null"), ({"o": None}, b"null"), ({"d": None}, b"null"),
                     ({"ln": None}, b"null"), ({"N": -1}, b"N"), ({"P": 0}, b"P"), ({"P": 4097}, b"P"), ({"pack_bytes": nb - 4}, b"pack_bytes"),
                     ({"H": 65}, b"H"), ({"C": 33}, b"C"), ({"n_hidden": 0}, b"hidden")):
        assert host(**kw) == -1 and text in L.isr_last_error(), kw
    # the device entries refuse before any device is touched (the pointers here are host arrays: never dereferenced)
    dbase = dict(pack=vp(pack), pack_bytes=nb, packT=vp(packT), packT_bytes=nbt, n_hidden=2, widths=vp(w), H=4, Wc=40, C=3, o=vp(o), d=vp(d),
                 ln=vp(ln), N=4, P=5, dd=None, dc=None, dW=vp(dW), db=vp(db), ws=vp(ws), ws_bytes=wsb(4, 5), stream=None)
    dev = lambda **kw: L.isr_radiance_backward(*{**dbase, **kw}.values())
    for kw, text in (({"pack": None}, b"null"), ({"packT": None}, b"null"), ({"widths": None}, b"null"), ({"o": None}, b"null"),
                     ({"ln": None}, b"null"), ({"ws": None}, b"null"), ({"ws_bytes": wsb(1, 64) - 256}, b"ws_bytes"), ({"ws_bytes": 0}, b"ws_bytes"),
                     ({"packT_bytes": nbt - 4}, b"packT_bytes"), ({"pack_bytes": nb + 4}, b"pack_bytes"), ({"N": -1}, b"N"),
                     ({"P": 4097}, b"P"), ({"Wc": 257}, b"Wc")):
        assert dev(**kw) == -1 and text in L.isr_last_error(), kw
    fr = dr.frequencies(4)
    pbase = dict(n_hidden=2, widths=vp(w), H=4, Wc=40, C=3, freqs=vp(fr), beta=10.0, W=vp(dW), b=vp(db), pack=vp(pack), pack_bytes=nb,
                 packT=vp(packT), packT_bytes=nbt, stream=None)
    packd = lambda **kw: L.isr_radiance_pack_device(*{**pbase, **kw}.values())
    for kw in ({"W": None}, {"b": None}, {"freqs": None}, {"pack": None}, {"packT": None}, {"pack_bytes": nb - 4}, {"packT_bytes": nbt + 4},
               {"beta": 0.0}, {"beta": float("inf")}, {"H": 0}):
        assert packd(**kw) == -1 and L.isr_last_error(), kw
    assert L.isr_radiance_grad_slopes_host(None, 3, 10.0, vp(ws), vp(ws)) == -1 and L.isr_radiance_grad_slopes_host(None, 0, 10.0, None, None) == 0


def test_wrappers_refuse_host_tensors(hip_lib):
    with pytest.raises(_capi.IsrError):
        ops.radiance_pack_device((5,), 4, 5, 3, dr.frequencies(4), 10.0, torch.zeros(8), torch.zeros(8))
    with pytest.raises(_capi.IsrError):
        ops.radiance_backward(torch.zeros(8), torch.zeros(8), (5,), 4, 5, 3, torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 2), None, None)


def test_ctypes_table_matches_the_header(hip_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "isr_radiance_grad.h").read_text(), flags=re.S)
    decls = dict(re.findall(r"\b(isr_[a-z0-9_]+)\s*\(([^)]*)\)", text))
    assert sorted(decls) == sorted(_capi.RADIANCE_GRAD_SIGNATURES) and len(decls) == 7
    for name, params in decls.items():
        assert hasattr(hip_lib, name), f"{name} declared in isr_radiance_grad.h but not exported"
        assert len(_capi.RADIANCE_GRAD_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    assert not set(_capi.RADIANCE_GRAD_SIGNATURES) & set(_capi.SIGNATURES)           # isr_hip.h's table stays what it is


class _Model(torch.nn.Module):
    """A module of NeuralRadianceFieldFeat's shape (nerf.py:163-218) without the reference: the names state_dict gives."""

    def __init__(self, H=4, hidden=8):
        super().__init__()
        sp = lambda: torch.nn.Softplus(beta=10.0)
        self.harmonic_embedding = torch.nn.Module()
        self.harmonic_embedding.register_buffer("frequencies", fields.DensityField.harmonic_frequencies(H))
        self.mlp = torch.nn.Sequential(torch.nn.Linear(6 * H, hidden), sp(), torch.nn.Linear(hidden, hidden), sp())
        self.color_layer = torch.nn.Sequential(torch.nn.Linear(hidden + 6 * H, hidden), sp(), torch.nn.Linear(hidden, 3), torch.nn.Sigmoid())
        self.feature_layer = torch.nn.Sequential(torch.nn.Linear(6 * H, hidden), sp(), torch.nn.Linear(hidden, 12), torch.nn.Sigmoid())
        self.density_layer = torch.nn.Sequential(torch.nn.Linear(hidden, 1), sp())


def test_trainable_radiance_field_on_the_cpu(hip_lib):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import TrainableRadianceField
    torch.manual_seed(5)
    model = _Model()
    fld = TrainableRadianceField.from_module(model, device="cpu")
    assert not isinstance(fld, fields.RadianceField) and isinstance(fld, torch.nn.Module)
    assert fld.widths == (8, 8) and (fld.H, fld.Wc, fld.C) == (4, 8, 3) and fld.beta == 10.0
    assert sorted(fld.state_dict()) == sorted([f"{k}.{i}" for k, n in (("weights", 3), ("biases", 3), ("color_weights", 2), ("color_biases", 2))
                                               for i in range(n)] + ["frequencies"])
    assert all(p.requires_grad for p in fld.parameters()) and len(list(fld.parameters())) == 10
    assert torch.equal(fld.weights[1], model.mlp[2].weight) and fld.weights[1] is not model.mlp[2].weight      # copies
    # the checkpoint's names, round trip bit for bit; feature_layer.* is ignored on load
    sd, want = fld.reference_state_dict(), model.state_dict()
    assert sorted(sd) == sorted(k for k in want if not k.startswith("feature_layer."))
    assert all(torch.equal(sd[k], want[k]) for k in sd)
    other = TrainableRadianceField.from_module(_Model(), device="cpu")
    assert not torch.equal(other.weights[0], fld.weights[0])
    other.load_reference_state_dict({"epoch": 3, "model_state_dict": want})
    assert all(torch.equal(a, b) for a, b in zip(other.parameters(), fld.parameters()))
    with pytest.raises(KeyError):
        other.load_reference_state_dict({k: v for k, v in want.items() if k != "color_layer.2.bias"})
    with pytest.raises(ValueError):
        other.load_reference_state_dict({**want, "mlp.0.weight": torch.zeros(3, 3)})
    # from_linears copies too, with RadianceField's signature
    lin = TrainableRadianceField.from_linears([model.mlp[0], model.mlp[2]], model.density_layer[0], [model.color_layer[0], model.color_layer[2]],
                                              n_harmonic=4, device="cpu")
    assert all(torch.equal(a, b) for a, b in zip(lin.parameters(), fld.parameters())) and torch.equal(lin.frequencies, fld.frequencies)
    # the frozen field of the current weights renders what a RadianceField of the same weights renders
    frozen = fld.to_radiance_field()
    assert frozen.device is None
    direct = fields.RadianceField(
        [m.weight for m in (model.mlp[0], model.mlp[2], model.density_layer[0])], [m.bias for m in (model.mlp[0], model.mlp[2], model.density_layer[0])],
        [model.color_layer[0].weight, model.color_layer[2].weight], [model.color_layer[0].bias, model.color_layer[2].bias],
        model.harmonic_embedding.frequencies, 10.0, None)
    o, d, ln = rr.bundle(5, 7)
    a, b = frozen.render_host(o, d, ln), direct.render_host(o, d, ln)
    assert all(rr.same(a[k], b[k]) for k in a)
    back = TrainableRadianceField.from_radiance_field(frozen, device="cpu")
    assert all(torch.equal(x, y) for x, y in zip(back.parameters(), fld.parameters()))
    # refusals
    bundle = type("B", (), {})()
    bundle.origins, bundle.directions, bundle.lengths = torch.from_numpy(o), torch.from_numpy(d), torch.from_numpy(ln)
    with pytest.raises(_capi.IsrError):
        fld(bundle)                                                            # CPU tensors: there is no CPU fallback
    bundle.lengths = bundle.lengths.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        fld(bundle)
    W = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError):
        TrainableRadianceField([W(8, 24), W(2, 8)], [W(8), W(2)], [W(8, 32), W(3, 8)], [W(8), W(3)], dr.frequencies(4))      # two densities
    with pytest.raises(ValueError):
        TrainableRadianceField([W(8, 24), W(1, 8)], [W(8), W(1)], [W(8, 30), W(3, 8)], [W(8), W(3)], dr.frequencies(4))      # W1's width
    with pytest.raises(ValueError):
        TrainableRadianceField([W(8, 24), W(1, 8)], [W(8), W(1)], [W(8, 32)], [W(8)], dr.frequencies(4))
    with pytest.raises(_capi.IsrError):
        TrainableRadianceField([W(8, 24), W(1, 8)], [W(8), W(1)], [W(8, 32), W(40, 8)], [W(8), W(40)], dr.frequencies(4))      # C > 32
    with pytest.raises(ValueError):
        TrainableRadianceField.from_linears([torch.nn.Linear(24, 8, bias=False)], torch.nn.Linear(8, 1),
                                            [torch.nn.Linear(32, 8), torch.nn.Linear(8, 3)], n_harmonic=4)
