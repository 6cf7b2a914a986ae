"""Shared by test_ref_fields_cpu.py and test_gpu_ref_fields.py (not a test module): the five fixtures that
tests/golden/make_ref_fields.py made by executing the reference's own classes and statements, the fields rebuilt from their
stored parameters, and the rules both files apply to them.  Nothing here reads the reference checkout.

Which rays may be left out is decided from the fixture alone, never from a result:
  a threshold-mode comparison leaves a ray out only if one of its stored f64 densities lies within 4 E_ref of the threshold;
  a distance filter leaves a ray out only if its stored f64 distance lies within 1e-6 of the cut;
  at most 1 % of a fixture's rays (CAP), asserted where the masks are made.

The point bound.  The reference forms a surface point as fl(o + fl(d t)) (two roundings); a fused kernel forms fl(o + d t).
With u = 2^-24:  |fl(d t) - d t| <= u |d t|, and each final rounding moves its sum by at most u times that sum, so the two
results differ by at most u (|d t| + |o + fl(d t)| + |o + d t|) <= u (|d t| + 2 |p|) (1 + 2u) per component, p the stored
point.  point_bound() evaluates that in f64 from the fixture's own o, d, t and p, with the factor (1 + 2^-20) for the
second-order terms; it is about 1.5 ulp of the point."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

G = Path(__file__).resolve().parent / "golden"
NAMES = ("ref_density_net", "ref_front_march", "ref_pc_grid", "ref_view_cors", "ref_key_export")
CAP = 0.01
f32, f64 = np.float32, np.float64
bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
_cache = {}


def load(name):
    if name not in _cache:
        with np.load(G / f"{name}.npz", allow_pickle=False) as z:
            _cache[name] = {k: z[k] for k in z.files}
        for a in _cache[name].values():
            a.setflags(write=False)
    return _cache[name]


def linears(g, tag):
    """torch.nn.Linear modules rebuilt from the stored arrays -> (hidden linears, density linear)."""
    mods = []
    for w, b in ((f"{tag}_W0", f"{tag}_b0"), (f"{tag}_W1", f"{tag}_b1"), (f"{tag}_Wd", f"{tag}_bd")):
        m = torch.nn.Linear(g[w].shape[1], g[w].shape[0])
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(g[w].copy()))
            m.bias.copy_(torch.from_numpy(g[b].copy()))
        mods.append(m)
    return mods[:2], mods[2]


def host_field(g, tag):
    """A host-only DensityField of the stored parameters; its frequencies are the ones from_linears would compute."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
    key = ("host field", id(g), tag)
    if key not in _cache:
        hidden, dens = linears(g, tag)
        mods = hidden + [dens]
        H = len(g[f"{tag}_frequencies"])
        _cache[key] = DensityField([m.weight for m in mods], [m.bias for m in mods], DensityField.harmonic_frequencies(H), 10.0, None)
    return _cache[key]


def device_field(g, tag, device):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import DensityField
    key = ("device field", id(g), tag, str(device))
    if key not in _cache:
        hidden, dens = linears(g, tag)
        _cache[key] = DensityField.from_linears(hidden, dens, n_harmonic=len(g[f"{tag}_frequencies"]), device=device)
    return _cache[key]


def point_bound(o, d, t, p):
    o, d, t, p = (np.asarray(a, f64) for a in (o, d, t, p))
    return 2.0 ** -24 * (np.abs(d * t[..., None]) + 2.0 * np.abs(p)) * (1.0 + 2.0 ** -20)


def assert_points(got, o, d, t, p, keep=None):
    """got within point_bound of the stored points p = o + d t, rows `keep` (all when None) -> the largest excess ratio."""
    err = np.abs(np.asarray(got, f64) - np.asarray(p, f64))
    bound = point_bound(o, d, t, p)
    if keep is not None:
        err, bound = err[keep], bound[keep]
    assert np.all(err <= bound), f"points: {int((err > bound).sum())} components past the two-roundings bound, worst {err.max():.3e}"
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def view_masks():
    """D's excused rays -> dict of boolean masks over the n rays of the bundle (front: density near 0.2 or distance near the
    cut; back: the same for the back march, placed at the rays idx1 names) and `any`; the cap is asserted."""
    g = load("ref_view_cors")
    e = 4 * float(g["E_ref"])
    n = g["origins"].shape[1]
    front_rho = (np.abs(g["front_dens64"][0, :, :, 0] - 0.2) <= e).any(axis=1)
    front_dist = np.abs(g["pdist1"][:, 0] - 0.1) <= 1e-6
    back_rho, back_dist = np.zeros(n, bool), np.zeros(n, bool)
    back_rho[g["idx1"]] = (np.abs(g["back_dens64"][0, :, :, 0] - 0.05) <= e).any(axis=1)
    back_dist[g["idx1"]] = np.abs(g["pdist2"][:, 0] - 0.1) <= 1e-6
    m = dict(front_rho=front_rho, front_dist=front_dist, back_rho=back_rho, back_dist=back_dist)
    m["any"] = front_rho | front_dist | back_rho | back_dist
    assert m["any"].mean() <= CAP, f"{int(m['any'].sum())} of {n} rays excused"
    return m


def check_view_sets(idx1, idx2, label):
    """idx1 (into the bundle) and idx2 (into the idx1 rays) of a run against D's, as sets of rays outside the excused ones."""
    g, m = load("ref_view_cors"), view_masks()
    idx1, idx2 = np.asarray(idx1), np.asarray(idx2)
    keep = lambda r: set(r[~m["any"][r]].tolist())
    ref2, got2 = g["idx1"][g["idx2"]], idx1[idx2]
    assert keep(idx1) == keep(g["idx1"]), f"{label}: idx1 differs outside the excused rays"
    assert keep(got2) == keep(ref2), f"{label}: idx2 differs outside the excused rays"
    return got2, ref2


def view_depths():
    """D's depths from its stored one-hot weights (the products are exact): front (n,) and back (n1,), f32."""
    g = load("ref_view_cors")
    P = int(g["rayCT"])
    front = (g["lengths"][0] * g["weights"][0]).max(axis=1)
    back = (g["backRaysLengths"][0] * g["backWeights"][0][:, P:]).max(axis=1)
    return front.astype(f32), back.astype(f32)


def check_saved(vc, got_idx1, got_ray2, label):
    """The four tensors of a whole run (dict of arrays xys, pos_vec, pos_vec_back, xys_back, batch 1) against D's saved ones:
    dtypes, shapes, and per common ray the xys bit for bit, the front points within point_bound, the back points within
    point_bound plus the front bound (their origin is the run's own front point)."""
    g, m = load("ref_view_cors"), view_masks()
    ref_ray2 = g["idx1"][g["idx2"]]
    t_front, t_back = view_depths()
    b_front = point_bound(g["origins"][0], g["directions"][0], t_front, g["posVec_all"][0])                       # (n, 3)
    b_back = np.zeros_like(b_front)
    b_back[g["idx1"]] = point_bound(g["posVec"][0], g["back_directions"][0], t_back, g["posVecBack_all"][0])
    for name, ref_name, rays_got, rays_ref, bound in (("xys", "saved_xys", got_idx1, g["idx1"], None),
                                                      ("pos_vec", "saved_posVec", got_idx1, g["idx1"], b_front),
                                                      ("pos_vec_back", "saved_posVecBack", got_ray2, ref_ray2, b_front + b_back),
                                                      ("xys_back", "saved_xys_back", got_ray2, ref_ray2, None)):
        a, r = np.asarray(vc[name]), g[ref_name]
        assert a.dtype == r.dtype and a.shape == (1, len(rays_got), r.shape[2]), f"{label}: {name} {a.dtype} {a.shape}"
        common = np.intersect1d(rays_got[~m["any"][rays_got]], rays_ref[~m["any"][rays_ref]])
        assert len(common) >= 0.9 * len(rays_ref)
        ga = a[0][np.searchsorted(rays_got, common)]
        ra = r[0][np.searchsorted(rays_ref, common)]
        if bound is None:
            assert np.array_equal(bits(ga), bits(ra)), f"{label}: {name}"
        else:
            assert np.all(np.abs(ga.astype(f64) - ra) <= bound[common]), f"{label}: {name}"


def bundle(g, device=None):
    t = lambda a: torch.from_numpy(a.copy()) if device is None else torch.from_numpy(a.copy()).to(device)
    return SimpleNamespace(origins=t(g["origins"]), directions=t(g["directions"]), lengths=t(g["lengths"]), xys=t(g["xys"]))
