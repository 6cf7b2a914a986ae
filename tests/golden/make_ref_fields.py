#!/usr/bin/env python3
"""Generates the five fixtures that pin the density-field stages to the reference's EXECUTED code:

  ref_density_net.npz   A  HarmonicEmbedding nerf.py:106-144 and NeuralRadianceFieldFeat nerf.py:148-767 (the class as it
                           stands; used of it: __init__ and _get_densities :148-228, customForwardForDensity :417-432,
                           forwardWithPoints :750-767, batched_forward_fordensity / forward_fordensity :523-638)
  ref_front_march.npz   B  the front marcher pren.py:338-365, the depth and the drop rule genFeat.py:191-198
  ref_pc_grid.npz       C  the marching-cubes input nerf.py:676-697, the argument expression of :700, statement :701
  ref_view_cors.npz     D  one view of generateCors.py:306-356 on the CPU, as the script's own .cpu() calls make it
  ref_key_export.npz    E  genFeat.py:204, :212-217, :223 (diamScaling from :72)

Runs on the build machine only (it reads the reference checkout).  As make_golden_from_reference.py does, nothing of the
reference is imported or stored: the files are parsed with `ast`, the named classes / the statements of the cited line ranges
are compiled and executed, and only DATA is written (numeric arrays; `_save` refuses anything else, so no fixture can hold
text).  Every range is guarded by needles, every class by the line numbers of its methods: a shifted range fails loudly.
The archives are written with a fixed time stamp, so a second run gives the same bytes.

Stand-ins.  pytorch3d, mcubes and trimesh are absent.  What the executed code needs of them is supplied here FROM MEMORY; it
is not the reference's text and it is NOT PINNED:
  .cuda()                     a no-op on tensors (torch.Tensor.cuda is patched inside `no_cuda()`, in this script only); the
                              executed statements use no .to(device)
  RayBundle                   a namedtuple of origins, directions, lengths, xys
  ray_bundle_to_ray_points    origins[..., None, :] + lengths[..., :, None] * directions[..., None, :]
  _shifted_cumprod            as in make_ref_back_march.py
  _check_raymarcher_inputs, _check_density_bounds   no-ops (they lie outside the executed ranges)
  KDTree                      sklearn.neighbors.KDTree: the reference's own call, not a stand-in
  mnormals                    trimesh's vertex normals enter E as input data
  Siren, Callable, Tuple, Union   names the class body mentions; siren=False never calls Siren

Re-parameterisation.  The reference's initial density bias of -1.5 gives densities of 0 or 1.19e-7 everywhere, which
discriminates nothing.  After construction the density row is rescaled and its bias set as tests/density_ref.fixture does
(A, C: half of [-1.2, 1.2]^3 above 0.2), or fitted by least squares to 6 (0.36 - |x|^2) (D: a blob of radius about 0.6 that
rays enter and leave).  That edits parameter DATA; no reference code is changed.

The f64 values.  `dens64` is the module after .double() on the f32 inputs widened, as it stands: there the embedding argument
x * f is an f64 product.  At H = 60 that is ANOTHER FUNCTION than the f32 module (f reaches 5.8e16, the f32 rounding of the
product is many periods), so for the (60, 256) net `E_ref` against it is of the order of the densities themselves and bounds
nothing.  `dens64_same_args` is the same .double() module's mlp and _get_densities on the sines and cosines of the f32
module's own embedding arguments, widened (the one line nerf.py:143 restated here); `E_ref_same_args` is the bound that
bites.  Both are stored and both are asserted.

Run from the repo root:  python tests/golden/make_ref_fields.py
"""
import ast
import collections
import contextlib
import copy
import io
import json
import sys
import types
import zipfile
from pathlib import Path
from typing import Callable, Tuple, Union

import numpy as np
import torch
from sklearn.neighbors import KDTree

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_from_reference import OUT, _stmts_in, _tree, ref_statements      # noqa: E402
from make_ref_back_march import _shifted_cumprod, marcher_code                     # noqa: E402

f32, f64 = np.float32, np.float64
RayBundle = collections.namedtuple("RayBundle", "origins directions lengths xys")
GRID_IDX = (0, 1, 2, 31, 63, 64, 65, 96, 125, 126, 127)
LINE_AT = (1, 31, 96)
CAP = 0.01                                  # the share of a fixture's rays that may be excused


def ray_bundle_to_ray_points(rb):
    return rb.origins[..., None, :] + rb.lengths[..., :, None] * rb.directions[..., None, :]


@contextlib.contextmanager
def no_cuda():
    orig = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = orig


def _save(name, out):
    """np.savez_compressed with a fixed time stamp; numeric arrays only; no larger than the largest fixture there is."""
    path = OUT / name
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            a = np.asarray(out[k])
            assert a.dtype.kind in "fiub", f"{name}: {k} has dtype {a.dtype}: fixtures hold numbers only, no text"
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a, order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    size, limit = path.stat().st_size, (OUT / "ref_assembly.npz").stat().st_size
    assert size <= limit, f"{name}: {size} bytes, more than ref_assembly.npz ({limit})"
    print(f"wrote {path.name}: {size} bytes, {len(out)} arrays")


def ref_class(fname, name, lineno, methods, needles, ns):
    """Compile ONE top-level `class name` of a reference file into `ns`; its line and its methods' lines are checked."""
    for node in _tree(fname).body:
        if isinstance(node, ast.ClassDef) and node.name == name:
            assert node.lineno == lineno, f"{fname}: class {name} at line {node.lineno}, expected {lineno}"
            at = {m.name: (m.lineno, m.end_lineno) for m in node.body if isinstance(m, ast.FunctionDef)}
            for m, span in methods.items():
                assert at.get(m) == span, f"{fname}: {name}.{m} at {at.get(m)}, expected {span}"
            text = ast.unparse(node)
            for needle in needles:
                assert needle in text, f"{fname}: class {name}: expected `{needle}`"
            exec(compile(ast.Module(body=[node], type_ignores=[]), f"{fname}:{name}", "exec"), ns)
            return ns[name]
    raise KeyError(f"{fname}: class {name} not found")


def ref_classes():
    ns = {"torch": torch, "np": np, "RayBundle": RayBundle, "ray_bundle_to_ray_points": ray_bundle_to_ray_points, "Siren": None,
          "Callable": Callable, "Tuple": Tuple, "Union": Union}
    ref_class("nerf.py", "HarmonicEmbedding", 106, {"__init__": (107, 133), "forward": (135, 144)},
              ("register_buffer", "omega0 * 2.0 ** torch.arange(n_harmonic_functions)", "x[..., None] * self.frequencies",
               "torch.cat((embed.sin(), embed.cos()), dim=-1)"), ns)
    return ref_class("nerf.py", "NeuralRadianceFieldFeat", 148,
                     {"__init__": (149, 218), "_get_densities": (220, 228), "customForwardForDensity": (417, 432),
                      "batched_forward_fordensity": (523, 586), "forward_fordensity": (587, 638),
                      "batched_forward_forPC": (640, 749), "forwardWithPoints": (750, 767)},
                     ("torch.nn.Softplus(beta=10.0)", "self.density_layer[0].bias.data[0] = -1.5", "1 - (-raw_densities).exp()",
                      "torch.nn.Linear(n_hidden_neurons, 1)", "ray_bundle_to_ray_points(ray_bundle)"), ns)


def _embed_args(model, x):
    """nerf.py:143 restated: the f32 module's embedding arguments."""
    return (x[..., None] * model.harmonic_embedding.frequencies).view(*x.shape[:-1], -1)


def same_args64(model, m64, x):
    e = _embed_args(model, x).double()
    return m64._get_densities(m64.mlp(torch.cat((e.sin(), e.cos()), dim=-1)))


@torch.no_grad()
def _hidden64(model, x):
    m64 = copy.deepcopy(model).double()
    e = _embed_args(model, x).double()
    return m64.mlp(torch.cat((e.sin(), e.cos()), dim=-1))


@torch.no_grad()
def reparam_half(model, rng):
    """tests/density_ref.fixture's rule on the module's own output row: the pre-activation's median where the density is 0.2
    (z = 0.2117), its spread 0.5, over 512 calibration points in [-1.2, 1.2]^3."""
    x = torch.from_numpy(rng.uniform(-1.2, 1.2, (512, 3)).astype(f32))
    lin = model.density_layer[0]
    row = lin.weight.data[0].double()
    u = _hidden64(model, x) @ row
    s = 0.5 / u.std(unbiased=False)
    lin.weight.data[0] = (row * s).float()
    lin.bias.data[0] = float(0.2117 - u.median() * s)


@torch.no_grad()
def reparam_blob(model, rng):
    """The output row and bias by least squares, so that the pre-activation is 6 (0.36 - |x|^2) over [-1.6, 1.6]^3."""
    x = torch.from_numpy(rng.uniform(-1.6, 1.6, (20000, 3)).astype(f32))
    h = _hidden64(model, x).numpy()
    z = 6.0 * (0.36 - (x.double().numpy() ** 2).sum(axis=1))
    sol = np.linalg.lstsq(np.concatenate([h, np.ones((len(h), 1))], axis=1), z, rcond=None)[0]
    lin = model.density_layer[0]
    lin.weight.data[0] = torch.from_numpy(sol[:-1]).float()
    lin.bias.data[0] = float(sol[-1])


def net_arrays(model, tag):
    g = lambda t: t.detach().numpy().copy()
    return {f"{tag}_W0": g(model.mlp[0].weight), f"{tag}_b0": g(model.mlp[0].bias), f"{tag}_W1": g(model.mlp[2].weight),
            f"{tag}_b1": g(model.mlp[2].bias), f"{tag}_Wd": g(model.density_layer[0].weight),
            f"{tag}_bd": g(model.density_layer[0].bias), f"{tag}_frequencies": g(model.harmonic_embedding.frequencies)}


def front_marcher_code():
    return ref_statements("pren.py", 338, 365, ("rays_densities = rays_densities[..., 0]", "if self.thresholdMode",
                                               "c1[torch.where(rays_densities > self.threshold)] = 1", "_shifted_cumprod(",
                                               "weights = rays_densities * absorption"))


def front_weights(code, rho, threshold, double=False):
    """pren.py:338-365 on densities (..., P, 1); threshold None: plain emission-absorption."""
    ns = {"torch": torch, "_shifted_cumprod": _shifted_cumprod, "eps": 1e-10,
          "self": types.SimpleNamespace(thresholdMode=threshold is not None, weightMode=False, threshold=threshold,
                                        surface_thickness=1),
          "rays_densities": (rho.double() if double else rho).clone()}
    exec(code, ns)
    return ns["weights"]


# ------------------------------------------------------------------------------------------------------------------ A
def make_density_net(NRF):
    rng = np.random.default_rng(20261101)
    torch.manual_seed(20261101)
    big, small = NRF(), NRF(n_harmonic_functions=4, n_hidden_neurons=32)
    out = {}
    pts = rng.uniform(-1.2, 1.2, (2049, 3)).astype(f32)
    pts[0], pts[1] = 0.0, -0.0
    pts[2:10] = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], f32)            # the grid's corners
    pts[10:18] = np.array([[x, y, z] for x in (-1.2, 1.2) for y in (-1.2, 1.2) for z in (-1.2, 1.2)], f32)
    for k in range(3):
        pts[18 + k, k] = 1e-30
    pts[21] = [1.0, -0.0, 1e-30]
    out["points"] = pts
    x = torch.from_numpy(pts)
    for model, tag in ((big, "big"), (small, "small")):
        assert not model.siren
        reparam_half(model, rng)
        out.update(net_arrays(model, tag))
        m64 = copy.deepcopy(model).double()
        with torch.no_grad():
            a, b = model.customForwardForDensity(x), model.forwardWithPoints(x)[0]
            d64 = m64.customForwardForDensity(x.double())
            d64s = same_args64(model, m64, x)
        assert torch.equal(a, b) and a.dtype == torch.float32 and d64.dtype == torch.float64 and a.shape == (2049, 1)
        share = float((a > 0.2).float().mean())
        assert 0.3 <= share <= 0.7, f"{tag}: {share:.2f} of the points above 0.2"
        out[f"{tag}_dens32"], out[f"{tag}_dens32_forwardWithPoints"] = a.numpy(), b.numpy()
        out[f"{tag}_dens64"], out[f"{tag}_dens64_same_args"] = d64.numpy(), d64s.numpy()
        out[f"{tag}_E_ref"] = f64((a.double() - d64).abs().max().item())
        out[f"{tag}_E_ref_same_args"] = f64((a.double() - d64s).abs().max().item())
        print(f"A {tag}: share above 0.2 {share:.2f}, E_ref {out[f'{tag}_E_ref']:.3e}, same arguments "
              f"{out[f'{tag}_E_ref_same_args']:.3e}")
        assert 0 < out[f"{tag}_E_ref_same_args"] < 1e-4
    _save("ref_density_net.npz", out)
    return small


# ------------------------------------------------------------------------------------------------------------------ B
def make_front_march():
    rng = np.random.default_rng(20261102)
    code = front_marcher_code()
    drop = ref_statements("genFeat.py", 191, 198, ("torch.max(sampled_rays1.lengths * weightsNeg, dim=-1)[0].unsqueeze(-1)",
                                                   "torch.where(torch.norm(negVec1 - sampled_rays1.origins, dim=-1)[0])[0]",
                                                   "negVec1 = negVec1[:, idx2]",
                                                   "fullNegVec = torch.cat([fullNegVec, negVec1.cpu()], dim=1)"))
    depth_expr = compile("torch.max(sampled_rays1.lengths * weightsNeg, dim=-1)[0]", "genFeat.py:193", "eval")   # its factor
    P, out = 24, {}
    bundles = []
    for b, R in enumerate((48, 20)):
        amp = rng.choice(np.array([0.02, 0.15, 0.6], f32), size=R, p=[0.2, 0.25, 0.55])
        rho = (rng.uniform(0.0, 1.0, (1, R, P)).astype(f32) * amp[None, :, None]).astype(f32)
        lengths = np.sort(rng.uniform(0.0, 1.5, (1, R, P)).astype(f32), axis=-1)
        if b == 0:
            rho[0, 0] = 0.01                                     # no sample above either threshold
            rho[0, 1] = 0.5                                      # every sample above them
            rho[0, 2, :-1], rho[0, 2, -1] = 0.01, 0.5            # only the last
            rho[0, 3, 1:], rho[0, 3, 0] = 0.01, 0.5              # only the first, at length 0: a hit at depth 0, dropped
            lengths[0, 3, 0] = 0.0
            rho[0, 4] = 0.2                                      # exactly genFeat's threshold: not above
            rho[0, 5] = 0.03                                     # exactly the class default
            lengths[0, 6] = -lengths[0, 6]                       # negative lengths
            rho[0, 6, 3] = 0.5
        o = rng.uniform(-0.5, 0.5, (1, R, 3)).astype(f32)
        d = rng.normal(size=(1, R, 3)).astype(f32)
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        bundles.append((o, d, lengths, rho))
        out.update({f"origins_b{b}": o, f"directions_b{b}": d, f"lengths_b{b}": lengths, f"rho_b{b}": rho})
    out["thresholds"] = np.array([0.2, 0.03], f64)
    for tag, thr in (("t020", 0.2), ("t003", 0.03), ("soft", None)):
        full = torch.Tensor([])                                  # genFeat.py:157
        hits = []
        for b, (o, d, ln, rho) in enumerate(bundles):
            rb = RayBundle(*(torch.from_numpy(a) for a in (o, d, ln)), None)
            w = front_weights(code, torch.from_numpy(rho)[..., None], thr)
            ns = {"torch": torch, "sampled_rays1": rb, "weightsNeg": w, "fullNegVec": full}
            dep = eval(depth_expr, ns)
            before = rb.origins + rb.directions * dep.unsqueeze(-1)
            exec(drop, ns)
            full = ns["fullNegVec"]
            assert torch.equal(before[:, ns["idx2"]], ns["negVec1"])
            out.update({f"{tag}_weights_b{b}": w.numpy(), f"{tag}_depth_b{b}": dep.numpy(), f"{tag}_points_b{b}": before.numpy(),
                        f"{tag}_idx2_b{b}": ns["idx2"].numpy()})
            hits.append((w != 0).any(dim=-1).numpy().reshape(-1))
            if thr is None:
                w64 = front_weights(code, torch.from_numpy(rho)[..., None], thr, double=True)
                ns64 = {"torch": torch, "sampled_rays1": RayBundle(None, None, rb.lengths.double(), None), "weightsNeg": w64}
                out.update({f"{tag}_weights64_b{b}": w64.numpy(), f"{tag}_depth64_b{b}": eval(depth_expr, ns64).numpy()})
        out[f"{tag}_fullNegVec"] = full.numpy()
        hit = np.concatenate(hits)
        print(f"B {tag}: {hit.mean():.2f} of the rays hit, fullNegVec {tuple(full.shape)}")
        if thr is not None:
            assert hit.mean() >= 0.25 and (~hit).mean() >= 0.10
            assert 0 < full.shape[1] < int(hit.sum())             # the hit at depth 0 is dropped with the misses
    _save("ref_front_march.npz", out)


# ------------------------------------------------------------------------------------------------------------------ C
def make_pc_grid(small):
    grid = ref_statements("nerf.py", 676, 697, ("gridRes = 128", "np.linspace(-1, 1, gridRes)",
                                                "[z0, y0, x0] for x0 in arr for y0 in arr for z0 in arr",
                                                "self.forwardWithPoints(gridCoords.view(-1, 3)[batch_idx])",
                                                "torch.Size((gridRes, gridRes, gridRes))"))
    out700: list[ast.stmt] = []
    _stmts_in(_tree("nerf.py").body, 700, 701, out700)
    call, rescale = out700[0].value, out700[1]
    assert ast.unparse(call.func) == "mcubes.marching_cubes" and ast.unparse(call.args[1]) == "threshold"
    arg = call.args[0]
    assert ast.unparse(arg) == "rays_densities[:, :, :, 0].movedim(0, 2).movedim(1, 0).cpu().numpy()"
    assert ast.unparse(rescale) == "mvertices = (mvertices - 64) / 64"
    arg_code = compile(ast.Expression(body=arg), "nerf.py:700", "eval")
    out = {}
    res = {}
    for tag, model in (("32", small), ("64", copy.deepcopy(small).double())):
        ns = {"torch": torch, "np": np, "self": model}
        with no_cuda(), torch.no_grad():
            exec(grid, ns)
            res[tag] = eval(arg_code, ns)
        assert res[tag].shape == (128, 128, 128) and ns["gridRes"] == 128
    D2, D2_64, t = res["32"], res["64"], ns["t"]
    assert D2.dtype == f32 and D2_64.dtype == f64 and t.dtype == f64
    ix = np.array(GRID_IDX)
    sub = D2[np.ix_(ix, ix, ix)]
    n_same = 0
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for flips in range(8):
            ixs = [127 - ix if flips >> a & 1 else ix for a in range(3)]
            other = D2.transpose(perm)[np.ix_(*ixs)]
            n_same += int(np.array_equal(other, sub))
            assert (perm == (0, 1, 2) and flips == 0) or np.abs(other.astype(f64) - sub).max() > 1e-3
    assert n_same == 1
    i, j, k = LINE_AT
    out.update(t=t, idx=ix.astype(np.int64), line_at=np.array(LINE_AT, np.int64), D2_sub=sub, D2_sub64=D2_64[np.ix_(ix, ix, ix)],
               D2_line0=D2[:, j, k], D2_line1=D2[i, :, k], D2_line2=D2[i, j, :],
               D2_line0_64=D2_64[:, j, k], D2_line1_64=D2_64[i, :, k], D2_line2_64=D2_64[i, j, :])
    e = max(np.abs(out[f"D2_line{a}"].astype(f64) - out[f"D2_line{a}_64"]).max() for a in range(3))
    out["E_ref"] = f64(max(e, np.abs(sub.astype(f64) - out["D2_sub64"]).max()))
    share = float((sub > 0.05).mean())
    print(f"C: E_ref {out['E_ref']:.3e}, {share:.2f} of the sub-lattice above 0.05")
    assert 0.2 <= share <= 0.8
    v = np.random.default_rng(20261103).uniform(0.0, 127.0, (16, 3))
    v[0], v[1], v[2] = 0.0, 127.0, 64.0
    ns = {"mvertices": v.copy()}
    exec(compile(ast.Module(body=[rescale], type_ignores=[]), "nerf.py:701", "exec"), ns)
    out.update(mc_vertices_in=v, mc_vertices_out=ns["mvertices"])
    _save("ref_pc_grid.npz", out)


# ------------------------------------------------------------------------------------------------------------------ D
def fibonacci_sphere(n, r):
    i = np.arange(n) + 0.5
    phi, z = np.pi * (1 + 5 ** 0.5) * i, 1 - 2 * i / n
    s = np.sqrt(1 - z * z)
    return r * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def view_rays_jittered(n_side, P, rng):
    """tests/back_march_ref.view_rays with the eye moved per ray, so that the origins' norms differ from ray to ray."""
    u = np.linspace(-0.9, 0.9, n_side).astype(f32)
    gx, gy = np.meshgrid(u, u, indexing="xy")
    n = n_side * n_side
    target = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3) + rng.uniform(-0.02, 0.02, (n, 3)).astype(f32)
    o = (np.array([0.3, -0.4, 2.6], f32) + rng.uniform(-0.05, 0.05, (n, 3)).astype(f32)).astype(f32)
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    ln = np.tile(np.linspace(1.7, 3.6, P).astype(f32), (n, 1))
    return o, d, ln, np.stack([gx, gy], -1).reshape(-1, 2).astype(f32)


def make_view_cors(NRF, seed=20261104):
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    model = NRF(n_harmonic_functions=4, n_hidden_neurons=32)
    reparam_blob(model, rng)
    m64 = copy.deepcopy(model).double()
    P = 24
    o, d, ln, xys = view_rays_jittered(25, P, rng)
    n = len(o)
    verts = fibonacci_sphere(4000, 0.6)
    verts = verts[~((verts[:, 0] > 0.3) & (verts[:, 2] > 0))]          # a hole on the side the rays come from
    out = net_arrays(model, "blob")
    out.update(origins=o[None], directions=d[None], lengths=ln[None], xys=xys[None], verts=verts, rayCT=np.int64(P))
    tt = lambda a: torch.from_numpy(a)[None]
    rays = RayBundle(tt(o), tt(d), tt(ln), tt(xys))
    rays64 = RayBundle(*(a.double() for a in rays))
    march = front_marcher_code()
    back_code = marcher_code()

    def raymarcherBack(rays_densities, rays_features):
        ns = {"torch": torch, "_shifted_cumprod": _shifted_cumprod, "eps": 1e-10,
              "self": types.SimpleNamespace(thresholdMode=True, surface_thickness=1),
              "rays_densities": rays_densities, "rays_features": rays_features}
        exec(back_code, ns)
        return None, torch.cat([ns["weights"], ns["weights2"]], dim=-1)                        # prenBack.py:385

    with no_cuda(), torch.no_grad():
        front32 = model.batched_forward_fordensity(ray_bundle=rays)[0]
        front64 = m64.batched_forward_fordensity(ray_bundle=rays64)[0]
        weights = front_weights(march, front32, 0.2)
        out.update(front_dens32=front32.numpy(), front_dens64=front64.numpy(), weights=weights.numpy())
        ns = {"torch": torch, "np": np, "RayBundle": RayBundle, "sampled_rays": rays, "weights": weights, "rayCT": P,
              "tree2": KDTree(np.asarray(verts), leaf_size=2), "neural_radiance_field": model, "raymarcherBack": raymarcherBack}
        run = lambda lo, hi, *needles: exec(ref_statements("generateCors.py", lo, hi, needles), ns)
        run(306, 309, "sampled_rays.lengths * weights[:, :, 0:rayCT]", "tree2.query(posVec[0].cpu().numpy(), k=1)",
            "pdist1[:, 0] < 0.1")
        out.update(posVec_all=ns["posVec"].numpy().copy(), pdist1=ns["pdist1"].copy(), idx1=ns["idx1"].copy())
        run(311, 330, "posVec = posVec[:, idx1, :].cpu()", "sampled_rays.lengths[:, :, 0].unsqueeze(-1)) / 3",
            "-(sampled_rays.origins / torch.norm(sampled_rays.origins, dim=-1).unsqueeze(-1)).cuda()", "origins=posVec.cuda()")
        backRays = ns["backRays"]
        out.update(posVec=ns["posVec"].numpy().copy(), backRaysLengths=ns["backRaysLengths"].numpy().copy(),
                   back_directions=backRays.directions.numpy().copy(),
                   origin_norms=torch.norm(ns["sampled_rays"].origins, dim=-1).numpy().copy())
        run(331, 332, "neural_radiance_field.batched_forward_fordensity(ray_bundle=backRays)",
            "raymarcherBack(rays_densities=back_rays_densities")
        back32 = ns["back_rays_densities"]
        back64 = m64.batched_forward_fordensity(ray_bundle=RayBundle(*(a.double() for a in backRays)))[0]
        out.update(back_dens32=back32.numpy().copy(), back_dens64=back64.numpy(), backWeights=ns["backWeights"].numpy().copy())
        run(333, 334, "del back_rays_densities", "backRays.lengths * backWeights[:, :, rayCT:]")
        out["posVecBack_all"] = ns["posVecBack"].numpy().copy()
        run(336, 356, "tree2.query(posVecBack[0].cpu().numpy(), k=1)", "pdist2[:, 0] < 0.1", "posVecBack = posVecBack[:, idx2].cpu()",
            "xys=backRays.xys.cpu()[:, idx2]", "cpuray_bundle = RayBundle(")
    out.update(pdist2=ns["pdist2"].copy(), idx2=ns["idx2"].copy(),
               saved_xys=ns["cpuray_bundle"].xys.numpy(), saved_posVec=ns["posVec"].numpy(),                   # :358-359
               saved_posVecBack=ns["posVecBack"].numpy(), saved_xys_back=ns["cpuray_bundle_backRays"].xys.numpy())   # :360-361
    n1, n2 = len(out["idx1"]), len(out["idx2"])
    hit = (weights != 0).any(dim=-1).numpy()[0]
    out["E_ref"] = f64(max(np.abs(out["front_dens32"].astype(f64) - out["front_dens64"]).max(),
                           np.abs(out["back_dens32"].astype(f64) - out["back_dens64"]).max()))
    ex1 = (np.abs(out["front_dens64"][0, :, :, 0] - 0.2) <= 4 * out["E_ref"]).any(axis=1) | (np.abs(out["pdist1"][:, 0] - 0.1) <= 1e-6)
    ex2 = (np.abs(out["back_dens64"][0, :, :, 0] - 0.05) <= 4 * out["E_ref"]).any(axis=1) | (np.abs(out["pdist2"][:, 0] - 0.1) <= 1e-6)
    excused = ex1.copy()
    excused[out["idx1"][ex2]] = True
    x, y, z = (out["origins"][0][out["idx1"]][:, a] for a in range(3))
    plain = np.sqrt(x * x + y * y + z * z)
    print(f"D: n {n}, n1 {n1}, n2 {n2}, hit {hit.mean():.2f}, E_ref {out['E_ref']:.3e}, excused {int(excused.sum())}, "
          f"norms where the written f32 sum differs from torch.norm: {int((plain != out['origin_norms'][0]).sum())}")
    assert hit.mean() >= 0.25 and (~hit).mean() >= 0.10 and 0 < n2 < n1 < n
    assert excused.mean() <= CAP, "choose another seed: the reference alone leaves the cap"
    assert (plain != out["origin_norms"][0]).sum() >= 5
    assert out["saved_xys"].shape == (1, n1, 2) and out["saved_posVec"].shape == (1, n1, 3)
    assert out["saved_posVecBack"].shape == (1, n2, 3) and out["saved_xys_back"].shape == (1, n2, 2)
    _save("ref_view_cors.npz", out)


# ------------------------------------------------------------------------------------------------------------------ E
def make_key_export():
    rng = np.random.default_rng(20261105)
    M = 3000
    verts = fibonacci_sphere(2000, 0.6)                                    # f64, as (mvertices - 64) / 64 is
    normals = verts / np.linalg.norm(verts, axis=1, keepdims=True)          # what trimesh would be asked for: input data
    dirs = rng.normal(size=(M, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    radius = 0.6 + rng.normal(size=M) * 0.02
    radius[2000:2600] += rng.uniform(-0.3, 0.3, 600)                       # far from the mesh
    radius[2600:] = rng.uniform(1.0, 2.2, 400)                             # some outside the 1.2 box
    cand = (dirs * radius[:, None]).astype(f32)
    cand[2999] = [1.2, 0.0, 0.0]                                           # f32(1.2) < 1.2 in f32: false
    diam = json.loads('{"diameter": 172.063}')["diameter"]
    scaling = {}
    exec(ref_statements("genFeat.py", 72, 72, ("diamScaling = 1.8",)), scaling)
    ns = {"torch": torch, "np": np, "KDTree": KDTree, "fullNegVec": torch.from_numpy(cand)[None], "mverts": verts,
          "mnormals": normals, "diam": diam, "diamScaling": scaling["diamScaling"]}
    box = ref_statements("genFeat.py", 204, 204, ("torch.max(torch.abs(fullNegVec[0, :, :]), dim=-1)[0] < 1.2",))
    inner = [s for s in ast.walk(_tree("genFeat.py")) if isinstance(s, ast.Subscript) and getattr(s, "lineno", 0) == 204
             and ast.unparse(s) == "torch.where(torch.max(torch.abs(fullNegVec[0, :, :]), dim=-1)[0] < 1.2)[0]"]
    assert len(inner) == 1
    box_idx = eval(compile(ast.Expression(body=inner[0]), "genFeat.py:204", "eval"), ns).numpy()
    exec(box, ns)
    fn_box = ns["fnVec"].numpy().copy()
    exec(ref_statements("genFeat.py", 212, 217, ("KDTree(np.asarray(mverts), leaf_size=2)", "pdist1[:, 0] < 0.05",
                                                 "fnVec = fnVec[:, closeidx]", "mnormals[pind1[:, 0]][closeidx]")), ns)
    exec(ref_statements("genFeat.py", 223, 223, ("fnVec[0].cpu().numpy() * (diam / diamScaling)",)), ns)
    out = dict(candidates=cand, verts=verts, normals=normals, diam=f64(diam), diamScaling=f64(scaling["diamScaling"]),
               box_idx=box_idx, fnVec_box=fn_box, pdist1=ns["pdist1"], pind1=ns["pind1"], closeidx=ns["closeidx"],
               fnVec=ns["fnVec"].numpy(), fnormalsVec=ns["fnormalsVec"], surfacePointsScaled=ns["surfacePointsScaled"])
    near = np.abs(ns["pdist1"][:, 0] - 0.05) <= 1e-6
    print(f"E: {M} candidates, {len(box_idx)} in the box, {len(ns['closeidx'])} close; {int(near.sum())} within 1e-6 of the cut; "
          f"surfacePointsScaled {ns['surfacePointsScaled'].dtype}")
    assert len(ns["closeidx"]) < len(box_idx) < M and len(ns["closeidx"]) > M // 4 and near.mean() <= CAP
    assert 2999 not in box_idx
    _save("ref_key_export.npz", out)


def main():
    NRF = ref_classes()
    small = make_density_net(NRF)
    make_front_march()
    make_pc_grid(small)
    make_view_cors(NRF)
    make_key_export()


if __name__ == "__main__":
    main()
