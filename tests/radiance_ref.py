"""Shared by the radiance-field tests (not a test module): fixture weights, a NumPy restatement of csrc/field_radiance.hpp's
chains (the direction rule, the f32 fmaf chains of the trunk and the colour head, the render of a ray, one operation at a
time; the activations come from the library's _host entries, which tests/test_radiance_cpu.py holds to f64 on their own),
the same layers as a torch module, and the bundles the CPU and the GPU tests share."""
import ctypes
import functools

import numpy as np
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi, fields
from tests import density_ref as dr

f32, f64 = np.float32, np.float64
NETS = [(1, 32, 1, 32, 3), (4, 32, 2, 40, 1), (4, 256, 2, 256, 3), (60, 32, 2, 32, 32)]      # H, hidden, n_hidden, Wc, C


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == f32 else np.int32)


def same(a, b):
    """Bit for bit, every NaN equal to every NaN (a NaN's sign and payload are the hardware's)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != f32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


def fixture(H, hidden, n_hidden, Wc, C, seed=0):
    """density_ref.fixture's trunk (about half of a point set above 0.2) and a colour head U(-1, 1) / sqrt(in) whose second
    layer is scaled by 4 so that the colours spread over (0, 1).  -> (Ws, bs, cWs, cbs), f32."""
    Ws, bs = dr.fixture(H, hidden, n_hidden, seed)
    rng = np.random.default_rng(seed + 1000)
    K = hidden + 6 * H
    cWs = [(rng.uniform(-1, 1, (Wc, K)) / np.sqrt(K)).astype(f32), (4 * rng.uniform(-1, 1, (C, Wc)) / np.sqrt(Wc)).astype(f32)]
    cbs = [rng.uniform(-0.1, 0.1, Wc).astype(f32), rng.uniform(-0.5, 0.5, C).astype(f32)]
    return Ws, bs, cWs, cbs


@functools.lru_cache(maxsize=None)
def host_field(net, seed=0):
    """-> (RadianceField without a device, its weights)"""
    H = net[0]
    w = fixture(*net, seed=seed)
    return fields.RadianceField(w[0], w[1], w[2], w[3], dr.frequencies(H), 10.0, None), w


def device_field(net, device, seed=0):
    H = net[0]
    w = fixture(*net, seed=seed)
    return fields.RadianceField(w[0], w[1], w[2], w[3], dr.frequencies(H), 10.0, device)


def sincos_host(a):
    a = np.ascontiguousarray(a, f32)
    s, c = np.empty_like(a), np.empty_like(a)
    _capi.check(_capi.lib().isr_density_sincos_host(_vp(a), a.size, _vp(s), _vp(c)), "sincos")
    return s, c


def activations_host(z, beta):
    z = np.ascontiguousarray(z, f32)
    sp, de = np.empty_like(z), np.empty_like(z)
    _capi.check(_capi.lib().isr_density_activations_host(_vp(z), z.size, float(beta), _vp(sp), _vp(de)), "activations")
    return sp, de


def sigmoid_host(z):
    z = np.ascontiguousarray(z, f32)
    out = np.empty_like(z)
    _capi.check(_capi.lib().isr_radiance_sigmoid_host(_vp(z), z.size, _vp(out)), "sigmoid")
    return out


def normalize_host(d):
    d = np.ascontiguousarray(d, f32).reshape(-1, 3)
    out = np.empty_like(d)
    _capi.check(_capi.lib().isr_radiance_normalize_host(_vp(d), d.shape[0], _vp(out)), "normalize")
    return out


def normalize(d):
    """The direction rule, one f32 operation at a time."""
    d = np.asarray(d, f32)
    with np.errstate(all="ignore"):
        s = dr.fma32(d[:, 2], d[:, 2], dr.fma32(d[:, 1], d[:, 1], (d[:, 0] * d[:, 0]).astype(f32)))
        n = np.sqrt(s).astype(f32)
        m = np.where(n < f32(1e-12), f32(1e-12), n)
        return (d / m[:, None]).astype(f32)


def embed(x, freqs):
    a = (np.asarray(x, f32)[:, :, None] * np.asarray(freqs, f32)[None, None, :]).reshape(len(x), -1)      # d * H + i
    s, c = sincos_host(a)
    return np.concatenate([s, c], axis=1)


def chain(W, h, z):
    """z_j <- fmaf(W[j, k], h[k], z_j) for k ascending; W (O, K), h (N, K), z (N, O)"""
    for k in range(W.shape[1]):
        z = dr.fma32(W[None, :, k], h[:, k:k + 1], z)
    return z


def eval_points(weights, freqs, beta, origins, directions, lengths):
    """-> (densities (N, P), colours (N, P, C)) by the definition of include/isr_radiance.h."""
    Ws, bs, cWs, cbs = weights
    o, d, ln = (np.asarray(a, f32) for a in (origins, directions, lengths))
    N, P = ln.shape
    Wt = Ws[-1].shape[1]
    with np.errstate(all="ignore"):
        pts = (o[:, None, :] + (d[:, None, :] * ln[:, :, None]).astype(f32)).astype(f32).reshape(-1, 3)
        h = embed(pts, freqs)
        for W, b in zip(Ws[:-1], bs[:-1]):
            z = chain(W, h, np.broadcast_to(b[None, :], (len(pts), len(b))).astype(f32))
            h = activations_host(z, beta)[0]
        zd = chain(Ws[-1], h, np.broadcast_to(bs[-1][None, :], (len(pts), 1)).astype(f32))
        dens = activations_host(activations_host(zd, beta)[0], beta)[1][:, 0]
        e_dir = embed(normalize(d), freqs)
        u = chain(cWs[0][:, Wt:], e_dir, np.broadcast_to(cbs[0][None, :], (N, len(cbs[0]))).astype(f32))      # per ray
        z = chain(cWs[0][:, :Wt], h, np.repeat(u, P, axis=0))
        g = activations_host(z, beta)[0]
        z2 = chain(cWs[1], g, np.broadcast_to(cbs[1][None, :], (len(pts), len(cbs[1]))).astype(f32))
        col = sigmoid_host(z2)
    return dens.reshape(N, P), col.reshape(N, P, -1)


def render(lengths, rho, colours, threshold):
    """The render of include/isr_radiance.h, one ray and one operation at a time -> (image (N, F+1), weights, depth, hit)."""
    lengths, rho, colours = np.asarray(lengths, f32), np.asarray(rho, f32), np.asarray(colours, f32)
    N, P = rho.shape
    F = colours.shape[2]
    image = np.zeros((N, F + 1), f32)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        wts, depth, hit = dr.march(lengths, rho, threshold)
        for n in range(N):
            feat = np.zeros(F, f32)
            T = one
            for k in range(P):
                c = (one if rho[n, k] > f32(threshold) else f32(0.0)) if threshold >= 0 else rho[n, k]
                feat = dr.fma32(np.broadcast_to(wts[n, k], (F,)), colours[n, k], feat)
                T = f32(T * f32(one - c))
            image[n, :F] = feat
            image[n, F] = f32(one - T)
    return image, wts, depth, hit


def bundle(N, P, seed=0, zero_dir=True):
    """N rays towards the unit cube with P ascending lengths: every ray its own unnormalised direction, ray 1 (if any) a zero
    direction."""
    rng = np.random.default_rng(1000 * P + N + seed)
    o = rng.uniform(-1.5, 1.5, (N, 3)).astype(f32)
    d = (rng.standard_normal((N, 3)) * rng.uniform(0.3, 3.0, (N, 1))).astype(f32)
    if zero_dir and N > 1:
        d[1] = 0
    ln = np.sort(rng.uniform(0.0, 2.0, (N, P)), axis=1).astype(f32)
    return o, d, ln


class TorchRadiance(torch.nn.Module):
    """The reference's layers as framework calls (nerf.py:163-218, :230-268): mlp, density_layer, color_layer behind
    HarmonicEmbedding, for tools/bench_radiance.py's comparison."""

    def __init__(self, weights, freqs, beta=10.0):
        super().__init__()
        Ws, bs, cWs, cbs = weights

        def lin(W, b):
            m = torch.nn.Linear(W.shape[1], W.shape[0])
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(W))
                m.bias.copy_(torch.from_numpy(b))
            return m
        mods = []
        for W, b in zip(Ws[:-1], bs[:-1]):
            mods += [lin(W, b), torch.nn.Softplus(beta=beta)]
        self.mlp = torch.nn.Sequential(*mods)
        self.density_layer = torch.nn.Sequential(lin(Ws[-1], bs[-1]), torch.nn.Softplus(beta=beta))
        self.color_layer = torch.nn.Sequential(lin(cWs[0], cbs[0]), torch.nn.Softplus(beta=beta), lin(cWs[1], cbs[1]),
                                               torch.nn.Sigmoid())
        self.register_buffer("frequencies", torch.from_numpy(np.asarray(freqs, f32)))

    def embed(self, x):
        e = (x[..., None] * self.frequencies).view(*x.shape[:-1], -1)
        return torch.cat((e.sin(), e.cos()), dim=-1)

    @torch.no_grad()
    def forward(self, origins, directions, lengths):
        pts = origins[..., None, :] + directions[..., None, :] * lengths[..., :, None]
        feats = self.mlp(self.embed(pts))
        dens = 1 - (-self.density_layer(feats)).exp()
        e_dir = self.embed(torch.nn.functional.normalize(directions, dim=-1))
        e_dir = e_dir[..., None, :].expand(*feats.shape[:-1], e_dir.shape[-1])
        return dens, self.color_layer(torch.cat((feats, e_dir), dim=-1))


# ---------------------------------------------------------------------------------------------- the reference fixture
PARITY = dr.PARITY.parent / "radiance_parity.json"
CAP = 0.01                                           # make_ref_fields.CAP: the share of a fixture's rays that may be excused
THRESHOLD = 0.2


def ref_field(tag, device=None):
    """The fixture's net as a RadianceField: the trunk from ref_density_net.npz (tests/golden/make_ref_render.py asserts that
    it is the one it ran), the colour head from ref_radiance_render.npz, its first matrix from the stored bf16 bits."""
    from tests import ref_fields as rf
    g, t = rf.load("ref_radiance_render"), rf.load("ref_density_net")
    Wc1 = (g[f"{tag}_Wc1_bf16"].astype(np.uint32) << 16).view(f32)
    Ws, bs = [t[f"{tag}_W0"], t[f"{tag}_W1"], t[f"{tag}_Wd"]], [t[f"{tag}_b0"], t[f"{tag}_b1"], t[f"{tag}_bd"]]
    H = len(t[f"{tag}_frequencies"])
    return fields.RadianceField(Ws, bs, [Wc1, g[f"{tag}_Wc2"]], [g[f"{tag}_bc1"], g[f"{tag}_bc2"]],
                                fields.DensityField.harmonic_frequencies(H), 10.0, device)


def check_against_reference(tag, soft, thr, who):
    """The conditions of the reference fixture on a soft render and a threshold render ({image, weights, densities, colours}
    as NumPy) of the fixture's bundle.  -> the measured ratios, also merged into profiles/radiance_parity.json under `who`."""
    import json
    from tests import ref_fields as rf
    g = rf.load("ref_radiance_render")
    e_col, e_img, e_dens = (float(g[f"{tag}_E_ref_{k}"]) for k in ("col", "image", "dens"))
    c64, d64 = g[f"{tag}_col64"][0], g[f"{tag}_dens64"][0, :, :, 0]
    assert e_col == float(np.abs(g[f"{tag}_col32"][0].astype(f64) - c64).max()) > 0
    assert e_img == float(np.abs(g[f"{tag}_soft_image32"][0].astype(f64) - g[f"{tag}_soft_image64"][0]).max()) > 0
    r_col = float(np.abs(soft["colours"].astype(f64) - c64).max()) / e_col
    r_dens = float(np.abs(soft["densities"].astype(f64) - d64).max()) / e_dens
    r_img = float(np.abs(soft["image"].astype(f64) - g[f"{tag}_soft_image64"][0]).max()) / e_img
    # threshold mode: a ray may be excused only if a stored f64 density lies within 4 E_ref of the threshold
    near = (np.abs(d64 - THRESHOLD) <= 4 * e_dens).any(axis=1)
    assert near.mean() <= CAP
    keep = ~near
    w32 = g[f"{tag}_thr_weights32"][0]
    assert np.array_equal(thr["weights"][keep], w32[keep])
    assert np.array_equal(thr["image"][keep, -1], g[f"{tag}_thr_image32"][0][keep, -1])
    # a threshold image is the colour of the chosen sample (or 0): the per-point colours' bound is its bound
    r_thr = float(np.abs(thr["image"][keep, :-1].astype(f64) - g[f"{tag}_thr_image64"][0][keep, :-1]).max()) / e_col
    rec = {"E_ref_colours": e_col, "E_ref_soft_image": e_img, "E_ref_densities": e_dens, "colours_over_E_ref": r_col,
           "densities_over_E_ref": r_dens, "soft_image_over_E_ref": r_img, "threshold_image_over_E_ref_colours": r_thr,
           "rays_excused": int(near.sum()), "rays": int(len(near))}
    print(f"{who} {tag}: {rec}")
    data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
    data.setdefault(who, {})[f"{tag} net"] = rec
    PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    assert r_col <= 4 and r_img <= 4 and r_thr <= 4 and r_dens <= 4, rec
    return rec
