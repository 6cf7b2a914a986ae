"""CPU: the bits of the host entries of the radiance field, of the emission-absorption march and its backward, and of the
march of given densities (isr_radiance_pack, isr_radiance_render_host, isr_ea_march_host, isr_ea_march_backward_host,
isr_density_march_given_host), pinned by tests/golden/radiance_host_bits.npz.  The file was written once by
tests/golden/make_radiance_host_bits.py, before the density and the radiance field came to share one trunk and one weight
chain: whatever is moved between those files, every entry must still give these words.  tests/test_field_bits_cpu.py pins
the density entries and lends its integer-only inputs (lcg), its nets' trunks, its rays and pack_digests.
A NaN is pinned as a NaN: its sign and payload are the hardware's (csrc/field_density.hpp), and differ between the fmaf of
a CPU with the instruction and the C library's, so every NaN word is stored and compared as 0x7fc00000."""
from pathlib import Path

import numpy as np
import pytest

from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import RadianceField
from tests import test_field_bits_cpu as fb

GOLDEN = Path(__file__).resolve().parent / "golden" / "radiance_host_bits.npz"
f32 = np.float32

# name -> (the trunk of test_field_bits_cpu.DENSITY_FIELDS, Wc, C, seed of the colour head)
RADIANCE_FIELDS = {"radiance_odd": ("density_odd", 40, 5, 303), "radiance_ref": ("density_ref", 256, 3, 302)}
THRESHOLDS = fb.THRESHOLDS
NON_FINITE_RAY = 3                     # its origin's first coordinate is +Inf: every point of the ray is not finite
MARCH_F, MARCH_P = (1, 13, 64), (1, 33)
MARCH_SCALE = (1.0, 0.15)              # of a ray's densities: the second ray stays below the threshold, the first need not
MARCH_N, MARCH_SEED = len(MARCH_SCALE), 41
DIRECTIONS = ("front", "back", "both")


def radiance_field(name):
    trunk, Wc, C, seed = RADIANCE_FIELDS[name]
    Ws, bs, freqs = fb.density_weights(trunk)
    K = Ws[-1].shape[1] + 6 * len(freqs)
    cWs = [(fb.lcg(seed, Wc * K) / np.sqrt(K)).astype(f32).reshape(Wc, K),
           (fb.lcg(seed + 10, C * Wc) * 4.0 / np.sqrt(Wc)).astype(f32).reshape(C, Wc)]
    cbs = [(fb.lcg(seed + 1, Wc) * 0.1).astype(f32), (fb.lcg(seed + 11, C) * 0.5).astype(f32)]
    return RadianceField(Ws, bs, cWs, cbs, freqs, 10.0, None)


def rays():
    """test_field_bits_cpu's 5 rays x 33 samples, one of them with an origin that is not finite."""
    inp = fb.small_inputs()
    o = inp["origins"].copy()
    o[NON_FINITE_RAY, 0] = np.inf
    return o, inp["directions"], inp["lengths"]


def march_inputs(P, F):
    """densities in [0, scale of the ray) (N, P), features (N, P, F), dimage (N, F + 1), dweights (N, P), lengths (N, P)
    ascending"""
    N, s = MARCH_N, MARCH_SEED + 100 * P + F
    rho = (0.5 * (fb.lcg(s, N * P).reshape(N, P) + 1.0) * np.array(MARCH_SCALE)[:, None]).astype(f32)
    feat = fb.lcg(s + 1, N * P * F).astype(f32).reshape(N, P, F)
    dimage = fb.lcg(s + 2, N * (F + 1)).astype(f32).reshape(N, F + 1)
    dweights = fb.lcg(s + 3, N * P).astype(f32).reshape(N, P)
    ln = ((np.arange(P)[None, :] + 0.5 * (fb.lcg(s + 4, N * P).reshape(N, P) + 1.0)) * (1.5 / P)).astype(f32)
    return rho, feat, dimage, dweights, ln


def words(a):
    """uint32 words of an f32 array with every NaN as 0x7fc00000; other arrays as they are."""
    a = np.ascontiguousarray(a)
    if a.dtype != f32:
        return a
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = 0x7FC00000
    return w


def compute():
    """Every pinned result: name -> array (f32 results as words)."""
    out = {}
    o, d, ln = rays()
    for name in RADIANCE_FIELDS:
        f = radiance_field(name)
        out[f"{name}_pack_words"] = np.array([f.rpack_host.size], np.int64)
        out[f"{name}_pack_digests"] = fb.pack_digests(f.rpack_host)
        for thr in THRESHOLDS:
            for k, v in f.render_host(o, d, ln, thr).items():
                out[f"{name}_render_{thr:g}_{k}"] = words(v)
    for P in MARCH_P:
        for F in MARCH_F:
            rho, feat, dimage, dweights, mln = march_inputs(P, F)
            for thr in THRESHOLDS:
                tag = f"P{P}_F{F}_{thr:g}"
                image, wts = ops.ea_march_host(rho, feat, thr)
                dd, df = ops.ea_march_backward_host(rho, feat, dimage, dweights, thr)
                out[f"ea_march_{tag}_image"], out[f"ea_march_{tag}_weights"] = words(image), words(wts)
                out[f"ea_backward_{tag}_ddensities"], out[f"ea_backward_{tag}_dfeatures"] = words(dd), words(df)
                if F == MARCH_F[0]:
                    for way in DIRECTIONS:
                        for k, v in zip(("weights", "depth", "hit"), ops.density_march_given_host(mln, rho, thr, way)):
                            out[f"given_P{P}_{thr:g}_{way}_{k}"] = words(v)
    return out


@pytest.fixture(scope="module")
def pinned(hip_lib):
    return dict(np.load(GOLDEN)), compute()


def _compare(pinned, prefix):
    gold, got = pinned
    names = [k for k in got if k.startswith(prefix)]
    assert names
    for k in names:
        g, w = got[k], gold[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            print(f"{k}: {len(bad)} of {g.size} differ, first at {bad[:8].tolist()}: got {g[tuple(bad[0])]:#x}, pinned {w[tuple(bad[0])]:#x}")
        assert np.array_equal(g, w), k


def test_every_stored_array_is_recomputed(pinned):
    gold, got = pinned
    assert set(gold) == set(got)
    assert GOLDEN.stat().st_size < fb.GOLDEN.stat().st_size


def hits(res, name):
    """name -> {threshold: rays that hit}"""
    return {thr: int(res[f"{name}_render_{thr:g}_hit"].sum()) for thr in THRESHOLDS}


@pytest.mark.parametrize("name", list(RADIANCE_FIELDS))
def test_the_fixture_has_rays_that_hit_and_rays_that_miss(pinned, name):
    """At the threshold some rays hit and some do not, the ray that is not finite among the latter (NaN > threshold is
    false).  At threshold -1 a weight is the density times the transmittance, and 1 - exp(-softplus) is 0 only below
    beta z = -708, which no net here reaches: every finite ray hits, and the one that is not has NaN weights, which count."""
    gold, _ = pinned
    n = hits(gold, name)
    assert 0 < n[0.2] < 5 and gold[f"{name}_render_0.2_hit"][NON_FINITE_RAY] == 0
    assert n[-1.0] == 5
    nan = gold[f"{name}_render_-1_image"][NON_FINITE_RAY] == 0x7FC00000
    assert nan.all()


@pytest.mark.parametrize("P", MARCH_P)
def test_the_given_densities_hit_and_miss(pinned, P):
    """At the threshold the first ray hits and the second does not, whatever F seeds them; at -1 both do."""
    gold, _ = pinned
    for F in MARCH_F:
        assert (march_inputs(P, F)[0] > 0.2).any(axis=1).tolist() == [True, False]
    assert gold[f"given_P{P}_0.2_front_hit"].tolist() == [1, 0] and gold[f"given_P{P}_-1_front_hit"].tolist() == [1, 1]


@pytest.mark.parametrize("name", list(RADIANCE_FIELDS))
def test_pack_and_render_keep_their_bits(pinned, name):
    """A differing digest row r is a difference inside the pack's words [256 r, 256 r + 256)."""
    _compare(pinned, name + "_")


@pytest.mark.parametrize("P", MARCH_P)
def test_marches_keep_their_bits(pinned, P):
    for prefix in (f"ea_march_P{P}_", f"ea_backward_P{P}_", f"given_P{P}_"):
        _compare(pinned, prefix)
