"""The ray losses of include/isr_ray_losses.h restated in NumPy, operation by operation (test infrastructure): the distortion
loss (nutil.mip360loss) and the render loss (the Huber terms of trainNerfFine.py:314-336) with their gradients, the case makers
the CPU and the GPU tests share, the fixture tests/golden/ref_ray_losses.npz and the measured-margin record
profiles/ray_losses_parity.json.

Every f32 operation is a NumPy f32 operation and every f64 one a NumPy f64 one; the only fused operation of the rule,
acc + (double)w_j * (double)|ut_i - ut_j|, has an exact product (two f32 factors), so a NumPy multiply and add round once too.
MUTATIONS switches one deliberate error into the rule; tests/test_ray_losses_cpu.py shows that each fails a named test."""
import json
import os
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "ref_ray_losses.npz"
PARITY = ROOT / "profiles" / "ray_losses_parity.json"
PARITY_MARGIN = 4.0          # the project's standing bound: x the reference-f32's own deviation from its f64
f32, f64 = np.float32, np.float64
LANES, REDUCE = 64, 256
NAN = np.array([0x7FC00000], np.uint32).view(f32)[0]
MUTATIONS = {"keep the last weight": False, "signed difference": False, "no factor 2": False, "last column": False, "+xy": False}


def canonical(a):
    a = np.array(a, f32)
    a[np.isnan(a)] = NAN
    return a


def same(a, b) -> bool:
    """Bit equality of two f32 arrays (every NaN the rule writes is canonical, so NaNs compare by bits as well)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def reduce_all(v):
    """REDUCE ORDER: trees of 256 (missing leaves +0), level by level, in f64."""
    v = np.asarray(v, f64).reshape(-1)
    while True:
        L2 = -(-v.size // REDUCE)
        w = np.zeros(L2 * REDUCE, f64)
        w[:v.size] = v
        w = w.reshape(L2, REDUCE)
        s = REDUCE // 2
        while s:
            w = w[:, :s] + w[:, s:2 * s]
            s //= 2
        v = w[:, 0]
        if v.size == 1:
            return v[0]


def _mean(S, count):
    with np.errstate(all="ignore"):
        return canonical(f32(f64(S) / f64(count)))


# ---- the distortion loss
def _depths(lengths):
    """-> t (N, P), ut (N, K), delta (N, K), all f32."""
    l = np.asarray(lengths, f32)
    with np.errstate(all="ignore"):
        d = (l - l[:, :1]) + f32(0.0)
        mx = d[:, 0].copy()
        for k in range(d.shape[1]):                       # the running maximum: a NaN on either side stays
            take = (d[:, k] > mx) | np.isnan(d[:, k])
            mx = np.where(take, d[:, k], mx)
        t = d / mx[:, None]
        ut = (t[:, 1:] + t[:, :-1]) / f32(2.0)
        delta = t[:, 1:] - t[:, :-1]
    return t, ut, delta


def _inner(w, ut):
    """inner (N, K) f64: the chain over j ascending from +0 of acc + (double)w_j * (double)|ut_i - ut_j|."""
    acc = np.zeros(ut.shape, f64)
    with np.errstate(all="ignore"):
        for j in range(ut.shape[1]):
            diff = ut - ut[:, j:j + 1]                    # f32
            diff = diff if MUTATIONS["signed difference"] else np.abs(diff)
            acc = acc + w[:, j:j + 1].astype(f64) * diff.astype(f64)
    return acc


def _cut(lengths, weights):
    lengths, weights = np.asarray(lengths, f32), np.asarray(weights, f32)
    t, ut, delta = _depths(lengths)
    if MUTATIONS["keep the last weight"]:                 # w = weights, one more interval of width 0 at the far end
        ut = np.concatenate([ut, t[:, -1:]], axis=1)
        delta = np.concatenate([delta, np.zeros_like(t[:, -1:])], axis=1)
        return weights, ut, delta
    return weights[:, :-1], ut, delta


def distortion_forward(lengths, weights):
    """-> (ray_loss (N) f32, loss f32)."""
    w, ut, delta = _cut(lengths, weights)
    N, K = w.shape
    with np.errstate(all="ignore"):
        inner = _inner(w, ut)
        wd = w.astype(f64)
        term = wd * inner + ((wd * wd) * delta.astype(f64)) / 3.0
        pad = np.zeros((N, -(-K // LANES) * LANES), f64)
        pad[:, :K] = term
        lane = np.zeros((N, LANES), f64)
        for r in range(pad.shape[1] // LANES):            # LANE ORDER: term_i to accumulator i mod 64, i ascending
            lane = lane + pad[:, r * LANES:(r + 1) * LANES]
        s = LANES // 2
        while s:
            lane = lane[:, :s] + lane[:, s:2 * s]
            s //= 2
        ray = lane[:, 0]
        return canonical(ray.astype(f32)), _mean(reduce_all(ray), N)


def distortion_backward(lengths, weights, upstream=1.0):
    """-> dweights (N, P) f32."""
    w, ut, delta = _cut(lengths, weights)
    N, P = np.asarray(weights).shape
    with np.errstate(all="ignore"):
        c = f64(f32(upstream)) / f64(N)
        inner = _inner(w, ut)
        g = (1.0 if MUTATIONS["no factor 2"] else 2.0) * inner + (2.0 * (w.astype(f64) * delta.astype(f64))) / 3.0
        out = np.zeros((N, P), f32)
        out[:, :w.shape[1]] = canonical((c * g).astype(f32))[:, :P]
    if MUTATIONS["last column"]:
        out[:, P - 1] = out[:, P - 2]
    return out


# ---- the render loss
def nearest_pixel(v, size):
    """csrc/rays.hpp's nearest_pixel: round-half-even of ((-v + 1) / 2) (size - 1) in f32, -1 outside."""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        g = v if MUTATIONS["+xy"] else -v
        f = np.rint(((g + f32(1.0)) / f32(2.0)) * f32(size - 1))
        ok = (f >= 0) & (f <= f32(size - 1))
        return np.where(ok, np.where(ok, f, 0).astype(np.int64), -1)


def _differences(rendered, images, sils, xys):
    """d (B, n, F+1) f32: the render minus its targets at the rays."""
    rendered, images, sils, xys = (np.asarray(a, f32) for a in (rendered, images, sils, xys))
    B, H, W, F = images.shape
    ix, iy = nearest_pixel(xys[..., 0], W), nearest_pixel(xys[..., 1], H)
    inside = (ix >= 0) & (iy >= 0)
    b = np.arange(B)[:, None]
    full = np.concatenate([images, sils[..., None]], axis=-1)
    y = np.where(inside[..., None], full[b, np.where(inside, iy, 0), np.where(inside, ix, 0)], f32(0.0))
    with np.errstate(all="ignore"):
        return rendered - y.astype(f32)


def _huber_parts(d, s):
    with np.errstate(all="ignore"):
        z = d.astype(f64) / f64(s)
        z2 = z * z
        return z2, np.sqrt(1.0 + z2)


def render_loss_forward(rendered, images, sils, xys, scaling=0.1):
    """-> out (2) f32."""
    d = _differences(rendered, images, sils, xys)
    B, n, F1 = d.shape
    z2, q = _huber_parts(d, scaling)
    with np.errstate(all="ignore"):
        h = np.where(z2 < np.inf, (f64(scaling) * z2) / (1.0 + q), z2).reshape(B * n, F1)
    rc = np.zeros(B * n, f64)
    for ch in range(F1 - 1):                              # the chain over the colour channels, ascending from +0
        rc = rc + h[:, ch]
    return np.array([_mean(reduce_all(rc), f64(B * n) * f64(F1 - 1)), _mean(reduce_all(h[:, F1 - 1]), B * n)], f32)


def render_loss_backward(rendered, images, sils, xys, upstream=(1.0, 1.0), scaling=0.1):
    """-> drendered (B, n, F+1) f32."""
    d = _differences(rendered, images, sils, xys)
    B, n, F1 = d.shape
    z2, q = _huber_parts(d, scaling)
    up = np.asarray(upstream, f32).astype(f64)
    with np.errstate(all="ignore"):
        k = np.concatenate([np.full(F1 - 1, up[0] / (f64(B * n) * f64(F1 - 1))), [up[1] / f64(B * n)]])
        g = canonical(((k * d.astype(f64)) / (f64(scaling) * q)).astype(f32))
    g[d == 0] = f32(0.0)
    return g


# ---- the reference's expressions in torch (the GPU tests' and the benchmark's yardstick): tensor methods only, any dtype
def torch_formula(lengths, weights):
    """The distortion loss as the reference defines it, every pair stored: lengths (..., P), weights (..., P) -> 0-d."""
    w = weights[..., :-1]
    t = lengths - lengths[..., :1]
    t = t / t.max(dim=-1, keepdim=True).values
    mid = 0.5 * (t[..., 1:] + t[..., :-1])
    pairs = (mid.unsqueeze(-1) - mid.unsqueeze(-2)).abs()
    inter = (w * (pairs * w.unsqueeze(-2)).sum(-1)).sum(-1)
    intra = (w * w * (t[..., 1:] - t[..., :-1])).sum(-1) / 3
    return (inter + intra).mean()


def torch_render_terms(rendered, images, sils, xys, scaling=0.1):
    """trainNerfFine.py:314-326 for one render with torch's own ops: grid_sample (nearest, align_corners) at -xy, the smooth L1
    term, .abs().mean() -> (color_err, sil_err)."""
    import torch
    B, F = images.shape[0], images.shape[-1]
    full = torch.cat([images, sils[..., None]], dim=-1).permute(0, 3, 1, 2)
    at = torch.nn.functional.grid_sample(full, -xys.reshape(B, -1, 1, 2), align_corners=True, mode="nearest")
    at = at.permute(0, 2, 3, 1).reshape(B, -1, F + 1)
    h = (((1 + (rendered.reshape(B, -1, F + 1) - at) ** 2 / scaling ** 2).clamp(1e-4).sqrt() - 1) * scaling).abs()
    return h[..., :F].mean(), h[..., F].mean()


# ---- cases
def march_weights(rng, N, P, scale=1.0):
    """The weights of an emission-absorption march of random densities: w_k = rho_k prod_{j<k} (1 - rho_j)."""
    rho = (rng.random((N, P)) ** 3 * scale).clip(0, 1).astype(f32)
    T = np.cumprod(np.concatenate([np.ones((N, 1), f32), 1 - rho[:, :-1]], axis=1), axis=1, dtype=f32)
    return (rho * T).astype(f32)


def fine_depths(rng, N, P, lo=1.0, hi=4.0):
    """The fine pass's depths: half a linspace, half random samples, sorted."""
    a = np.broadcast_to(np.linspace(lo, hi, P // 2, dtype=f32), (N, P // 2))
    b = (lo + (hi - lo) * rng.random((N, P - P // 2))).astype(f32)
    return np.sort(np.concatenate([a, b], axis=1), axis=1).astype(f32)


def distortion_rows(rng, P):
    """The rows of the issue's list at P samples -> (lengths (9, P), weights (9, P)); row 4 is the all-equal one (NaN)."""
    lin = np.linspace(1.0, 4.0, P, dtype=f32)
    srt = np.sort(1 + 3 * rng.random(P)).astype(f32)
    uns = (1 + 3 * rng.random(P)).astype(f32)
    uns[0], uns[-1] = 1.5, 4.0                            # depths below the first one, and the largest is not the first (that is NaN)
    two = srt.copy()
    two[P // 2] = two[P // 2 - 1] if P > 2 else two[P // 2]
    eq = np.full(P, 2.5, f32)
    L = np.stack([lin, srt, uns, two, eq, lin, srt, fine_depths(rng, 1, P)[0], uns])
    Wt = march_weights(rng, 9, P)
    Wt[5] = 0                                             # all-zero weights
    Wt[6] = 0
    Wt[6, (P - 1) // 2] = 1                               # one-hot
    Wt[7, P // 3] = np.nan                                # a NaN weight
    Wt[8, ::2] = -0.0                                     # -0 weights
    return L, Wt


NAN_ROWS, CLEAN_ROWS = [4, 7], [0, 1, 2, 3, 5, 6, 8]     # of distortion_rows


def distortion_cases():
    """name -> (lengths, weights): every P of the issue over the nine rows, every N of the issue over mixed rows."""
    rng = np.random.default_rng(20261020)
    out = {}
    for P in (2, 3, 64, 65, 128, 257, 1024):
        out[f"P = {P}"] = distortion_rows(rng, P)
        out[f"P = {P}, the rows without a NaN"] = tuple(a[CLEAN_ROWS] for a in out[f"P = {P}"])      # a finite mean
    for N in (1, 2, 63, 64, 65, 129):
        L = fine_depths(rng, N, 33)
        L[N // 2:] = L[N // 2:, rng.permutation(33)]      # the second half unsorted
        out[f"N = {N}"] = (L, march_weights(rng, N, 33))
    return out


TREE_EDGES = (1, 256, 257, 65536, 65537)                  # REDUCE ORDER's level edges: one tree, two levels, three


def tree_edge_cases():
    """name -> (lengths, weights): N rays at every level edge of REDUCE ORDER, P = 2 (a ray's value is w_0^2 / 3)."""
    rng = np.random.default_rng(20261022)
    return {f"N = {N}, P = 2": (fine_depths(rng, N, 2), march_weights(rng, N, 2)) for N in TREE_EDGES}


UPSTREAMS = (1.0, -2.5, 0.0)
RENDER_UPSTREAMS = ((1.0, 1.0), (-2.5, 0.0), (0.0, 3.0))


def render_case(rng, B, n, F, H, W, special=True, nonfinite=False):
    """-> (rendered, images, sils, xys); special: rays outside on each side, exact half-integer positions and d = 0 entries;
    nonfinite: a NaN in rendered and huge d as well."""
    images = rng.random((B, H, W, F)).astype(f32)
    sils = (rng.random((B, H, W)) < 0.5).astype(f32)
    xys = (2.4 * rng.random((B, n, 2)) - 1.2).astype(f32)
    if special and n >= 12:
        xys[0, 0], xys[0, 1], xys[0, 2], xys[0, 3] = (1.5, 0.0), (-1.5, 0.0), (0.0, 1.5), (0.0, -1.5)
        if W > 1 and H > 1:                               # pixel positions k + 1/2 exactly: (g + 1) / 2 (size - 1) = k + 1/2
            xys[0, 4] = (-(2 * f32(0.5) / f32(W - 1) - 1), -(2 * f32(1.5) / f32(H - 1) - 1))
            xys[0, 5] = (-(2 * f32(2.5) / f32(W - 1) - 1) if W > 3 else 0.0, 0.0)
    rendered = rng.random((B, n, F + 1)).astype(f32)
    if special and n >= 12:
        d0 = _differences(np.zeros_like(rendered), images, sils, xys)      # minus the targets
        rendered[:, 6:9] = -d0[:, 6:9]                    # d = 0 exactly, colours and opacity
    if nonfinite:
        rendered[0, 9, 0] = np.nan
        rendered[0, 10, F] = 3e38
        rendered[0, 11, 0] = -1e30
    return rendered, images, sils, xys


def render_cases():
    rng = np.random.default_rng(20261021)
    out = {}
    for F in (1, 3, 12):
        out[f"F = {F}"] = render_case(rng, 2, 40, F, 9, 5)
    out["a NaN in rendered and huge d"] = render_case(rng, 2, 40, 3, 9, 5, nonfinite=True)
    out["H = 1"] = render_case(rng, 2, 40, 3, 1, 9)
    out["W = 1"] = render_case(rng, 2, 40, 3, 9, 1)
    out["one ray"] = render_case(rng, 1, 1, 3, 5, 5, special=False)
    out["past one tree"] = render_case(rng, 3, 257, 3, 8, 8)
    return out


def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def ulp32(x) -> float:
    return float(np.spacing(np.abs(f32(x))))


def record(section: str, values: dict) -> None:
    """Merge measured ratios into profiles/ray_losses_parity.json (only when ISR_RECORD_PARITY is set: tests do not write)."""
    if not os.environ.get("ISR_RECORD_PARITY"):
        return
    data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
    data.setdefault(section, {}).update(values)
    PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
