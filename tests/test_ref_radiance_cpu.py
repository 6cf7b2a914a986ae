"""CPU: the radiance field and its render against tests/golden/ref_radiance_render.npz, the results of the reference's
executed code (tests/golden/make_ref_render.py): NeuralRadianceFieldFeat.forward in mode="color", the raymarcher at
thresholdMode False and True, get_emb_vis and normImage.  The normalised directions bit for bit; per-point colours and
soft-mode images within 4 x the reference's own f32-to-f64 deviation; threshold mode with equal weights and opacity.
Measured (host build, ratio to E_ref, allowed 4): written to profiles/radiance_parity.json by the test."""
import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import render
from tests import radiance_ref as rr
from tests import ref_fields as rf


def test_fixture_holds_numbers_only_and_discriminates():
    g = rf.load("ref_radiance_render")
    assert all(a.dtype.kind in "fiu" for a in g.values())
    for tag, R, P in (("big", 125, 64), ("small", 250, 16)):
        assert g[f"{tag}_col32"].shape == (1, R, P, 3) and g[f"{tag}_soft_image32"].shape == (1, R, 4)
        d = g[f"{tag}_directions"][0]
        n = np.linalg.norm(d, axis=1)
        assert len(np.unique(d, axis=0)) == R and n.min() > 0.5 and n.max() > 2 * n.min()      # distinct, unnormalised
        assert 0.15 < (g[f"{tag}_dens32"] > 0.2).mean() < 0.85 and g[f"{tag}_col32"].std() > 0.01
        assert (g[f"{tag}_thr_image32"][0, :, 3] == 1).mean() > 0.3


@pytest.mark.parametrize("tag", ["big", "small"])
def test_normalised_directions_are_the_fixture_s(hip_lib, tag):
    g = rf.load("ref_radiance_render")
    got = rr.normalize_host(g[f"{tag}_directions"][0])
    assert np.array_equal(rr.bits(got), rr.bits(g[f"{tag}_directions_normed"][0]))


@pytest.mark.parametrize("tag", ["big", "small"])
def test_host_render_against_the_reference(hip_lib, tag):
    g = rf.load("ref_radiance_render")
    f = rr.ref_field(tag)
    o, d, ln = g[f"{tag}_origins"][0], g[f"{tag}_directions"][0], g[f"{tag}_lengths"][0]
    rr.check_against_reference(tag, f.render_host(o, d, ln, -1.0), f.render_host(o, d, ln, rr.THRESHOLD), "host build")


def test_image_helpers_equal_the_fixture():
    g = rf.load("ref_radiance_render")
    emb, mask = torch.from_numpy(g["vis_emb"].copy()), torch.from_numpy(g["vis_mask"].astype(bool))
    assert np.array_equal(render.get_emb_vis(emb.clone()).numpy(), g["vis_plain"])
    assert np.array_equal(render.get_emb_vis(emb.clone(), mask, True).numpy(), g["vis_masked_demeaned"])
    assert np.array_equal(render.normImage(emb.clone()).numpy(), g["vis_norm_image"])
