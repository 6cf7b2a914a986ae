"""Shared by the tests of the march's backward (not a test module): a NumPy restatement of include/isr_ea_grad.h — the rule one
operation at a time in f32, every fmaf exact (density_ref.fma32), vectorised over the rays and serial along each ray — the
reference's expression (pren.py:362-367) in torch for the comparisons in f64, the fixture of tests/golden/make_ref_ea_grad.py,
the bound both comparisons use, and the cases the CPU and the GPU tests share."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from .density_ref import fma32

f32, f64 = np.float32, np.float64
GOLDEN = Path(__file__).resolve().parent / "golden" / "ref_ea_grad.npz"
PARITY = Path(__file__).resolve().parent.parent / "profiles" / "ea_grad_parity.json"
MARGIN = 4.0                                           # times the reference-f32's own deviation from its f64: the standing margin
FIXTURES = ("train", "wide")


def backward_ref(rho, feat, dimage, dweights=None, threshold: float = -1.0):
    """rho (N, P), feat (N, P, F), dimage (N, F + 1), dweights (N, P) or None -> (ddensities, dfeatures, weights)."""
    rho, feat, dimage = np.asarray(rho, f32), np.asarray(feat, f32), np.asarray(dimage, f32)
    N, P, F = feat.shape
    one = f32(1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        c = np.where(rho > f32(threshold), one, f32(0)).astype(f32) if threshold >= 0 else rho
        T, t = np.empty((N, P), f32), np.ones(N, f32)
        for k in range(P):
            T[:, k] = t
            t = t * (one - c[:, k])
        w = c * T
        dfeat = w[:, :, None] * dimage[:, None, :F]
        if threshold >= 0:
            return np.zeros((N, P), f32), dfeat, w
        g = np.zeros((N, P), f32) if dweights is None else np.array(dweights, f32)
        for ch in range(F):
            g = fma32(np.broadcast_to(dimage[:, ch:ch + 1], (N, P)), feat[:, :, ch], g)
        dd, a = np.empty((N, P), f32), -dimage[:, F]
        for k in range(P - 1, -1, -1):
            dd[:, k] = T[:, k] * (g[:, k] - a)
            a = fma32(g[:, k], c[:, k], a * (one - c[:, k]))
    return dd, dfeat, w


def pren_march(dens: torch.Tensor, feat: torch.Tensor, eps: float = 1e-10):
    """pren.py:362-367 written in torch, with pytorch3d's _shifted_cumprod as tests/golden/make_ref_back_march.py supplies it:
    dens (N, P), feat (N, P, F) -> (image (N, F + 1), weights (N, P)).  Differentiable by torch."""
    cp = torch.cumprod((1.0 + eps) - dens, dim=-1)
    absorption = torch.cat([torch.ones_like(cp[..., :1]), cp[..., :-1]], dim=-1)
    weights = dens * absorption
    features = (weights[..., None] * feat).sum(dim=-2)
    opacities = 1.0 - torch.prod(1.0 - dens, dim=-1, keepdim=True)
    return torch.cat((features, opacities), dim=-1), weights


def fixture(tag: str) -> dict:
    """One shape of ref_ea_grad.npz: rho, feat, Wi (the image's contraction), Ww (the weights'), the reference's f64 gradients
    dd64 and df64, and E_dd, E_df: the largest deviation of the reference's own f32 gradients from them.  The file keeps
    feat as int8 sixty-fourths and df64 as its two exact factors (the generator asserts the product is the gradient)."""
    z = np.load(GOLDEN)
    g = lambda k: z[f"{tag}_{k}"]
    Wi = g("Wi")
    return {"rho": g("rho"), "feat": g("feat_q").astype(f32) / f32(64), "Wi": Wi, "Ww": g("Ww"), "dd64": g("dd64"),
            "df64": g("w64")[:, :, None] * Wi.astype(f64)[:, None, :-1], "E_dd": float(g("E_dd")), "E_df": float(g("E_df"))}


def bound(E_ref: float, want64) -> float:
    """MARGIN times the reference-f32's deviation from its f64, and at least one f32 ulp of the array's largest magnitude: the
    reference's eps = 1e-10 is not representable beside 1 in f32 but is in f64."""
    return max(MARGIN * E_ref, float(np.spacing(f32(np.abs(want64).max()))))


def densities(rng, kind: str, N: int, P: int):
    if kind == "uniform":
        return rng.uniform(0, 1, (N, P)).astype(f32)
    if kind == "small":
        return rng.uniform(0, 0.05, (N, P)).astype(f32)
    if kind == "sharp":                                # a surface: a sigmoid head across it
        x = np.linspace(-1, 1, P)[None, :] - rng.uniform(-0.5, 0.5, (N, 1))
        return (1 / (1 + np.exp(-40 * x))).astype(f32)
    raise KeyError(kind)


def random_case(rng, N: int, P: int, F: int, kind: str = "uniform", dweights: bool = True, threshold: float = -1.0):
    return (densities(rng, kind, N, P), rng.standard_normal((N, P, F)).astype(f32), rng.standard_normal((N, F + 1)).astype(f32),
            rng.standard_normal((N, P)).astype(f32) if dweights else None, threshold)


def cases():
    """name -> (rho, feat, dimage, dweights or None, threshold): the edge cases of the issue."""
    rng = np.random.default_rng(20261019)
    out = {}
    for P in (1, 2, 3, 64, 65, 257):
        for F in (1, 3, 16, 17, 33):
            out[f"P = {P}, F = {F}"] = random_case(rng, 5, P, F, ("uniform", "small", "sharp")[(P + F) % 3])
    rho, feat, dimage, dw, thr = random_case(rng, 6, 40, 3, "small")
    out["densities all 0"] = (np.zeros_like(rho), feat, dimage, dw, thr)
    out["densities all 1"] = (np.ones_like(rho), feat, dimage, dw, thr)
    mid = rho.copy()
    mid[:, 17], mid[2, 3] = 1.0, 1.0
    out["an exact 1 mid-ray"] = (mid, feat, dimage, dw, thr)
    out["densities above 1 and negative"] = (rng.uniform(-0.5, 1.5, rho.shape).astype(f32), feat, dimage, dw, thr)
    nan = rho.copy()
    nan[3, 11] = np.nan
    out["one NaN ray among clean rays"] = (nan, feat, dimage, dw, thr)
    bad = feat.copy()
    bad[1, 5, 2], bad[4, 30, 0] = np.nan, np.inf
    out["features with a NaN and an infinity"] = (rho, bad, dimage, dw, thr)
    out["dimage of zeros"] = (rho, feat, np.zeros_like(dimage), dw, thr)
    out["dimage of -0"] = (rho, feat, np.full_like(dimage, -0.0), None, thr)
    for name, v, at in (("a NaN", np.nan, (2, 1)), ("an infinity", np.inf, (4, 3))):
        d = dimage.copy()
        d[at] = v
        out[f"dimage with {name}"] = (rho, feat, d, dw, thr)
    out["dweights null"] = (rho, feat, dimage, None, thr)
    out["dweights of zeros"] = (rho, feat, dimage, np.zeros_like(dw), thr)
    for t in (0.02, 0.0, 2.0):
        out[f"threshold mode, {t}"] = (nan if t == 0.02 else rho, feat, dimage, dw, t)
    return out


def same_bits(a, b) -> bool:
    """Bit equality of two f32 arrays, -0 and +0 apart; a NaN equals a NaN (its payload is the arithmetic unit's business)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[keep], b.view(np.uint32)[keep])
