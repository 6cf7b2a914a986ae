"""CPU: the ray losses of include/isr_ray_losses.h.  The host build of csrc/ray_losses.hpp (the GPU tests' reference) against
the NumPy restatement tests/ray_losses_ref.py bit for bit, at every size edge and on every kind of row the header names; against
the reference's executed code (tests/golden/ref_ray_losses.npz) within 4 x the reference-f32's own deviation from its f64; the
mutations of the rule, each of which fails that comparison; the refusals; and the Python layer's argument checks."""
import re

import numpy as np
import pytest

from . import ray_losses_ref as ref

f32, f64 = np.float32, np.float64
DISTORTION = ref.distortion_cases()
RENDER = ref.render_cases()


@pytest.fixture(scope="module")
def ops(hip_lib):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    return ops


def test_header_and_table_agree(hip_lib):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", (ref.ROOT / "include" / "isr_ray_losses.h").read_text(), flags=re.S)
    decls = dict(re.findall(r"\b(isr_[a-z0-9_]+)\s*\(([^)]*)\)", text))
    assert sorted(decls) == sorted(_capi.RAY_LOSSES_SIGNATURES) and len(decls) == 11
    for name, params in decls.items():
        assert hasattr(hip_lib, name), name
        assert len(_capi.RAY_LOSSES_SIGNATURES[name][1]) == len([p for p in params.split(",") if p.strip()]), name
    assert not set(_capi.RAY_LOSSES_SIGNATURES) & set(_capi.SIGNATURES)                # isr_hip.h's table stays what it is
    main = re.sub(r"/\*.*?\*/", "", (ref.ROOT / "include" / "isr_hip.h").read_text(), flags=re.S)
    assert "isr_distortion" not in main and "isr_render_loss" not in main and hip_lib.isr_abi_version() == 6
    assert {k: hip_lib.isr_ray_losses_geometry(i) for i, k in enumerate(("group_rays", "lanes", "reduce", "max_p"))} == \
        {"group_rays": 4, "lanes": ref.LANES, "reduce": ref.REDUCE, "max_p": 1024}


@pytest.mark.parametrize("name", list(DISTORTION))
def test_distortion_host_is_the_restatement(ops, name):
    L, W = DISTORTION[name]
    ray_loss, loss = ops.distortion_forward_host(L, W)
    want_rays, want_loss = ref.distortion_forward(L, W)
    assert ref.same(ray_loss, want_rays) and ref.same(loss, want_loss)
    assert ref.same(ops.distortion_forward_host(L, W, want_ray_loss=False)[1], want_loss)      # ray_loss left out
    if "without a NaN" in name or name.startswith("N ="):
        assert np.isfinite(loss) and loss > 0
    elif name.startswith("P ="):
        assert np.isnan(ray_loss[ref.NAN_ROWS]).all() and np.isfinite(ray_loss[ref.CLEAN_ROWS]).all() and np.isnan(loss)
    for up in ref.UPSTREAMS:
        dw = ops.distortion_backward_host(L, W, up)
        assert ref.same(dw, ref.distortion_backward(L, W, up)), up
        assert not dw[:, -1].view(np.uint32).any()                                    # column P-1 is +0, NaN rows included


EDGES = ref.tree_edge_cases()


@pytest.mark.parametrize("name", list(EDGES))
def test_distortion_host_at_the_level_edges_of_the_ordered_sum(ops, name):
    """N = 1, 256, 257, 65 536 and 65 537 leaves: below, at and above one tree of 256 and two levels of trees."""
    L, W = EDGES[name]
    ray_loss, loss = ops.distortion_forward_host(L, W)
    want_rays, want_loss = ref.distortion_forward(L, W)
    assert ref.same(ray_loss, want_rays) and ref.same(loss, want_loss)
    assert np.isfinite(loss) and loss > 0


def test_two_samples_closed_form(ops):
    """P = 2: inter = 0 and intra = w_0^2 / 3, whatever the two ascending depths are."""
    L = np.array([[1.0, 4.0], [2.0, 2.5], [3.0, 7.0]], f32)
    W = np.array([[0.5, 9.0], [0.25, 9.0], [1.5, 9.0]], f32)
    ray_loss, loss = ops.distortion_forward_host(L, W)
    assert ref.same(ray_loss, (W[:, 0].astype(f64) ** 2 / 3.0).astype(f32))
    assert ref.same(ops.distortion_backward_host(L, W, 3.0), np.stack([(2.0 * W[:, 0].astype(f64) / 3.0).astype(f32), np.zeros(3, f32)], 1))


def test_a_row_alone_and_among_129(ops):
    """ray_loss and dweights of a row do not depend on its neighbours (upstream N keeps c = upstream / N at 1), and a NaN row
    changes no other row."""
    L, W = DISTORTION["N = 129"]
    rays, _ = ops.distortion_forward_host(L, W)
    dw = ops.distortion_backward_host(L, W, 129.0)
    for i in (0, 64, 128):
        alone, _ = ops.distortion_forward_host(L[i:i + 1], W[i:i + 1])
        assert ref.same(alone, rays[i:i + 1]) and ref.same(ops.distortion_backward_host(L[i:i + 1], W[i:i + 1], 1.0), dw[i:i + 1])
    L2 = L.copy()
    L2[64] = 2.5                                                                      # all depths equal: NaN
    rays2, loss2 = ops.distortion_forward_host(L2, W)
    dw2 = ops.distortion_backward_host(L2, W, 129.0)
    others = np.arange(129) != 64
    assert np.isnan(rays2[64]) and np.isnan(loss2) and np.isnan(dw2[64, :-1]).all() and dw2[64, -1] == 0
    assert ref.same(rays2[others], rays[others]) and ref.same(dw2[others], dw[others])


@pytest.mark.parametrize("name", list(RENDER))
def test_render_loss_host_is_the_restatement(ops, name):
    case = RENDER[name]
    out = ops.render_loss_forward_host(*case)
    assert ref.same(out, ref.render_loss_forward(*case))
    if "NaN" in name:
        assert np.isnan(out[0]) and out[1] > 1e30
    else:
        assert np.isfinite(out).all() and (out > 0).all()
    d = ref._differences(*case)
    for up in ref.RENDER_UPSTREAMS:
        g = ops.render_loss_backward_host(*case, up)
        assert ref.same(g, ref.render_loss_backward(*case, up)), up
        assert not g[d == 0].view(np.uint32).any()                                    # exactly +0 where d = 0
    if name == "F = 3":
        assert (d == 0).sum() >= 2 * 3 * 4                                            # the case does hold such entries
        ix = ref.nearest_pixel(case[3][0, :6, 0], 5)
        assert list(ix[:4]) == [-1, -1, 2, 2] and list(ix[4:6]) == [0, 2]             # outside left and right; halves go to even


def test_render_loss_scaling(ops):
    case = RENDER["F = 3"]
    for s in (0.1, 0.5, 3.0):
        assert ref.same(ops.render_loss_forward_host(*case, s), ref.render_loss_forward(*case, s))
        assert ref.same(ops.render_loss_backward_host(*case, (1.0, 2.0), s), ref.render_loss_backward(*case, (1.0, 2.0), s))


# ---- against the reference's executed code
def golden_ratios(distortion_forward, distortion_backward, render_forward, render_backward):
    """-> ({name: deviation / allowance}, every NaN where the reference has one): the deviation of each loss and each gradient
    array from the reference's f64 result, over PARITY_MARGIN x the reference-f32's own deviation (losses: at least one f32 ulp)."""
    fx = ref.fixture()
    ratios, nans = {}, True
    for tag in ("small", "coarse", "fine", "equal"):
        L, W = fx[f"{tag}_lengths"], fx[f"{tag}_weights"]
        loss = distortion_forward(L, W)[1]
        g, g64 = distortion_backward(L, W, 1.0).astype(f64), fx[f"{tag}_dweights_f64"]
        nans = nans and bool((np.isnan(g) == np.isnan(g64)).all()) and bool(np.isnan(loss) == np.isnan(fx[f"{tag}_loss_f64"]))
        if tag != "equal":
            allow = max(ref.PARITY_MARGIN * float(fx[f"{tag}_loss_eref"]), ref.ulp32(fx[f"{tag}_loss_f64"]))
            ratios[f"{tag} loss"] = abs(float(loss) - float(fx[f"{tag}_loss_f64"])) / allow
        ratios[f"{tag} dweights"] = float(np.nanmax(np.abs(g - g64))) / (ref.PARITY_MARGIN * float(fx[f"{tag}_dweights_eref"]))
    case = [fx[f"render_{k}"] for k in ("rendered", "images", "sils", "xys")]
    out = render_forward(*case).astype(f64)
    for v, what in enumerate(("colour", "silhouette")):
        allow = max(ref.PARITY_MARGIN * float(fx["render_out_eref"][v]), ref.ulp32(fx["render_out_f64"][v]))
        ratios[f"render {what}"] = abs(out[v] - fx["render_out_f64"][v]) / allow
    g = render_backward(*case, fx["render_upstream"]).astype(f64)
    ratios["render drendered"] = float(np.abs(g - fx["render_drendered_f64"]).max()) / (ref.PARITY_MARGIN * float(fx["render_drendered_eref"]))
    return ratios, nans


def test_against_the_references_executed_code(ops):
    """Every gradient array within 4 x the reference-f32's own deviation from its f64 result, every loss within the same or one
    f32 ulp; no entry is excused.  The measured multiples of the reference-f32's deviation go to profiles/ray_losses_parity.json
    when ISR_RECORD_PARITY is set."""
    ratios, nans = golden_ratios(ops.distortion_forward_host, ops.distortion_backward_host, ops.render_loss_forward_host,
                                 ops.render_loss_backward_host)
    for k, v in ratios.items():
        print(f"{k}: {v:.3f} of the allowance")
    assert nans and all(v <= 1.0 for v in ratios.values()), ratios
    ref.record("host build against the reference's executed code, multiples of the reference-f32's own deviation",
               {k: round(v * ref.PARITY_MARGIN, 3) for k, v in ratios.items() if not k.endswith("loss") and "render c" not in k
                and "render s" not in k})
    ref.record("host build against the reference's executed code, losses: fraction of max(4 x deviation, one f32 ulp)",
               {k: round(v, 3) for k, v in ratios.items() if k.endswith("loss") or "render c" in k or "render s" in k})


@pytest.mark.parametrize("mutation,caught_by", [("keep the last weight", "small dweights"), ("signed difference", "fine dweights"),
                                                ("no factor 2", "coarse dweights"), ("last column", "small dweights"),
                                                ("+xy", "render drendered")])
def test_mutations_fail_the_reference_comparison(monkeypatch, mutation, caught_by):
    """The restatement passes test_against_the_references_executed_code's comparison as it stands and fails it with any one of the
    rule's mutations: the dropped [:P-1] cut, a signed difference, the factor 2 on inner_i, a non-zero last column, +xy."""
    impl = (ref.distortion_forward, ref.distortion_backward, ref.render_loss_forward, ref.render_loss_backward)
    ratios, nans = golden_ratios(*impl)
    assert nans and all(v <= 1.0 for v in ratios.values())
    monkeypatch.setitem(ref.MUTATIONS, mutation, True)
    ratios, _ = golden_ratios(*impl)
    assert ratios[caught_by] > 1.0, ratios


def test_refusals(ops, hip_lib):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import IsrError
    ok = np.ones((3, 5), f32)
    for L, W, msg in ((np.ones((3, 1), f32), np.ones((3, 1), f32), "P outside"), (np.ones((2, 1025), f32), np.ones((2, 1025), f32), "P outside"),
                      (np.ones((0, 5), f32), np.ones((0, 5), f32), "N < 1")):
        for fn in (ops.distortion_forward_host, ops.distortion_backward_host):
            with pytest.raises(IsrError, match=msg):
                fn(L, W)
    assert hip_lib.isr_distortion_workspace_bytes(0, 5) == 0 and hip_lib.isr_distortion_workspace_bytes(5, 1) == 0
    assert hip_lib.isr_distortion_workspace_bytes(5, 1025) == 0 and hip_lib.isr_distortion_workspace_bytes(5, 1024) > 0
    p = ok.ctypes.data
    assert hip_lib.isr_distortion_forward_host(None, p, 3, 5, None, p) == -1 and b"null" in hip_lib.isr_last_error()
    assert hip_lib.isr_distortion_forward_host(p, p, 3, 5, None, None) == -1
    assert hip_lib.isr_distortion_backward_host(p, p, 3, 5, None, p) == -1 and hip_lib.isr_distortion_backward_host(p, p, 3, 5, p, None) == -1
    # the device entries check their arguments before they touch a device
    assert hip_lib.isr_distortion_forward(p, p, 3, 1, None, p, p, 1 << 20, None) == -1 and b"P outside" in hip_lib.isr_last_error()
    assert hip_lib.isr_distortion_forward(p, p, 3, 5, None, p, p, 8, None) == -1 and b"workspace" in hip_lib.isr_last_error()
    assert hip_lib.isr_distortion_forward(p, p, 3, 5, None, p, None, 0, None) == -1
    assert hip_lib.isr_distortion_backward(p, p, 3, 1025, p, p, None) == -1 and hip_lib.isr_distortion_backward(p, p, 3, 5, None, p, None) == -1
    case = RENDER["F = 3"]
    for s in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(IsrError, match="scaling"):
            ops.render_loss_forward_host(*case, s)
        with pytest.raises(IsrError, match="scaling"):
            ops.render_loss_backward_host(*case, (1.0, 1.0), s)
    with pytest.raises(ValueError):
        ops.render_loss_forward_host(case[0][..., :3], *case[1:])                      # F + 1 channels expected
    assert hip_lib.isr_render_loss_forward_host(p, p, p, None, 1, 1, 1, 1, 1, 0.1, p) == -1 and b"null" in hip_lib.isr_last_error()
    assert hip_lib.isr_render_loss_forward(p, p, p, p, 1, 1, 65, 1, 1, 0.1, p, p, 1 << 20, None) == -1 and b"F outside" in hip_lib.isr_last_error()
    assert hip_lib.isr_render_loss_forward(p, p, p, p, 1, 1, 1, 1, 1, 0.1, p, p, 8, None) == -1 and b"workspace" in hip_lib.isr_last_error()
    assert hip_lib.isr_render_loss_backward(p, p, p, p, 1, 1, 1, 1, 1, 0.1, None, p, None) == -1
    assert hip_lib.isr_render_loss_workspace_bytes(0, 5) == 0 and hip_lib.isr_render_loss_workspace_bytes(2, 600) >= 2 * 16


def test_python_layer_checks(hip_lib):
    import torch
    from types import SimpleNamespace
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import losses
    from imagesequenceregistrationfor6dposeestimationlabeling_amd._capi import IsrError
    L, W = torch.linspace(1, 4, 8).repeat(3, 1), torch.rand(3, 8)
    with pytest.raises(IsrError):
        losses.distortion_loss(L, W)                                                  # CPU tensors: no fallback
    with pytest.raises(IsrError):
        losses.mip360loss(SimpleNamespace(lengths=L), W)
    with pytest.raises(NotImplementedError):
        losses.distortion_loss(L.clone().requires_grad_(True), W)
    with pytest.raises(ValueError):
        losses.distortion_loss(L[:, :7], W)
    with pytest.raises(IsrError):
        losses.render_loss(torch.rand(2, 5, 4), torch.rand(2, 6, 6, 3), torch.rand(2, 6, 6), torch.rand(2, 5, 2))
    x, y = torch.rand(5), torch.rand(5)                                               # huber stays what it was
    assert torch.equal(losses.huber(x, y), ((1 + (x - y) ** 2 / (0.1 ** 2)).clamp(1e-4).sqrt() - 1) * 0.1)
