"""Shared by the density-field tests (not a test module): fixture weights, a NumPy restatement of csrc/field_density.hpp (the
f32 fmaf chain, softplus32, density32 and the march, one operation at a time), the same layers as torch modules with the
reference's cumprod march, and the measured-margin record profiles/density_field_parity.json."""
import json
from pathlib import Path

import numpy as np
import torch

PARITY = Path(__file__).resolve().parent.parent / "profiles" / "density_field_parity.json"
f32, f64 = np.float32, np.float64


def frequencies(H, omega0=0.1):
    """As HarmonicEmbedding builds them (nerf.py:131-134), f32 as torch rounds them."""
    return (omega0 * (2.0 ** torch.arange(H))).to(torch.float32).numpy()


def fixture(H, hidden, n_layers, seed=0):
    """Hidden layers U(-1, 1) / sqrt(in), biases U(-0.1, 0.1).  The output row is U(-1, 1) scaled, and its bias set, so that over
    512 calibration points in [-1.2, 1.2]^3 the pre-activation of the density has its median where the density is 0.2
    (z = 0.2117) and a spread of 0.5: about half of any such point set is above the threshold (the reference's initial bias
    of -1.5 with small weights gives densities near 3e-8 everywhere).  -> (Ws, bs) with the output row last, f32."""
    rng = np.random.default_rng(seed)
    w = [6 * H] + [hidden] * n_layers
    Ws = [(rng.uniform(-1, 1, (o, i)) / np.sqrt(i)).astype(f32) for i, o in zip(w[:-1], w[1:])]
    bs = [rng.uniform(-0.1, 0.1, o).astype(f32) for o in w[1:]]
    row = rng.uniform(-1, 1, (1, hidden))
    x = rng.uniform(-1.2, 1.2, (512, 3)).astype(f32)
    a = (x[:, :, None] * frequencies(H)[None, None, :]).reshape(512, -1).astype(f64)
    h = np.concatenate([np.sin(a), np.cos(a)], axis=1)
    for W, b in zip(Ws, bs):
        z = 10.0 * (h @ W.astype(f64).T + b.astype(f64))
        h = np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, 20)))) / 10.0
    u = h @ row[0]
    row = row * (0.5 / u.std())
    Ws.append(row.astype(f32))
    bs.append(np.array([0.2117 - np.median(u) * 0.5 / u.std()], f32))
    return Ws, bs


def fma32(a, b, c):
    """fmaf on f32 arrays, exactly: the f64 product of two f32 is exact; the f64 sum is rounded to odd (TwoSum tells whether it
    was inexact), and rounding that to f32 is then a single rounding (53 >= 2 * 24 + 2)."""
    p = a.astype(f64) * b.astype(f64)
    c = np.broadcast_to(c.astype(f64), p.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
    step = np.where((err > 0) == (s > 0), 1, -1)
    return np.where(fix, bits + step, bits).view(f64).astype(f32)


def _expm1_kernel(r):
    t = r * r
    c = r - t * (1.66666666666666019037e-01 + t * (-2.77777777770155933842e-03 + t * (6.61375632143793436117e-05 + t * (
        -1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))))
    return r - (r * c) / (c - 2.0)


def _reduce_ln2(x):
    kf = np.rint(x * 1.44269504088896338700e+00)
    return kf, (x - kf * 6.93147180369123816490e-01) - kf * 1.90821492927058770002e-10


def _pow2(kf):
    return ((kf.astype(np.int64) + 1023) << 52).view(f64)


def exp64(x):
    x = np.asarray(x, f64)
    nan, lo, hi = np.isnan(x), x < -708.0, x > 709.0
    xs = np.where(nan | lo | hi, 0.0, x)
    kf, r = _reduce_ln2(xs)
    y = _pow2(kf) * (1.0 + _expm1_kernel(r))
    return np.where(nan, x, np.where(lo, 0.0, np.where(hi, np.inf, y)))


def log1p64(y):
    y = np.asarray(y, f64)
    nan = np.isnan(y)
    ys = np.where(nan, 0.0, y)
    u = 1.0 + ys
    c = np.where(u >= 2.0, 1.0 - (u - ys), ys - (u - 1.0)) / u
    ub = u.view(np.int64)
    k = (ub >> 52) - 1023
    mant = ub & 0x000fffffffffffff
    big = mant >= 0x0006a09e667f3bcd
    k = k + big
    m = np.where(big, mant | 0x3fe0000000000000, mant | 0x3ff0000000000000).view(f64)
    f = m - 1.0
    hfsq = 0.5 * f * f
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01))
    t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)))
    R = t2 + t1
    dk = k.astype(f64)
    out = dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + (dk * 1.90821492927058770002e-10 + c))) - f)
    return np.where(nan, y, out)


def softplus32(z, beta):
    z = np.asarray(z, f32)
    t = f64(f32(beta)) * z.astype(f64)
    with np.errstate(invalid="ignore"):
        soft = (log1p64(exp64(np.where(t > 20.0, 0.0, t))) / f64(f32(beta))).astype(f32)
    return np.where(t > 20.0, z, soft)


def density32(s):
    s = np.asarray(s, f32)
    x = -s.astype(f64)
    nan, sat = np.isnan(x), x < -40.0
    xs = np.where(nan | sat, 0.0, x)
    kf, r = _reduce_ln2(xs)
    p = _expm1_kernel(r)
    tk = _pow2(kf)
    v = np.where(kf == 0, -p, -(tk * p + (tk - 1.0))).astype(f32)
    return np.where(nan, s, np.where(sat, f32(1.0), v))


def eval_points(Ws, bs, freqs, beta, pts, sincos):
    """The definition, per point (vectorised over points and neurons, the k loop in order).  sincos(a) -> (sin, cos) is the
    library's sincos32 (isr_density_sincos_host)."""
    pts = np.asarray(pts, f32)
    a = (pts[:, :, None] * np.asarray(freqs, f32)[None, None, :]).reshape(len(pts), -1)      # (N, 3H): d * H + i
    s, c = sincos(a)
    h = np.concatenate([s, c], axis=1)
    for l, (W, b) in enumerate(zip(Ws, bs)):
        z = np.broadcast_to(b[None, :], (len(pts), len(b))).astype(f32)
        for k in range(W.shape[1]):
            z = fma32(W[None, :, k], h[:, k:k + 1], z)
        h = softplus32(z, beta)
    return density32(h[:, 0])


def march(lengths, rho, threshold):
    """csrc/field_density.hpp's march_ray, one ray at a time -> (weights, depth, hit)."""
    lengths, rho = np.asarray(lengths, f32), np.asarray(rho, f32)
    N, P = lengths.shape
    wts, depth, hit = np.zeros((N, P), f32), np.zeros(N, f32), np.zeros(N, np.int32)
    one = f32(1.0)
    for n in range(N):
        absorb = one
        for k in range(P):
            if threshold >= 0:
                c = one if rho[n, k] > f32(threshold) else f32(0.0)
            else:
                c = rho[n, k]
            w = f32(c * absorb)
            absorb = f32(absorb * f32(one - c))
            wts[n, k] = w
            v = f32(lengths[n, k] * w)
            if k == 0:
                m = v
            elif not np.isnan(m) and (np.isnan(v) or v > m):
                m = v
        depth[n] = m
        hit[n] = int(np.any(wts[n] != 0))
    return wts, depth, hit


def surface(origins, directions, depth):
    return (np.asarray(origins, f32) + (np.asarray(directions, f32) * np.asarray(depth, f32)[:, None]).astype(f32)).astype(f32)


class TorchDensity(torch.nn.Module):
    """The reference's layers as framework calls (nerf.py:163-177, :206-228): Sequential(Linear, Softplus(beta), ...) and
    1 - exp(-x), behind HarmonicEmbedding's forward (nerf.py:143-144)."""

    def __init__(self, Ws, bs, freqs, beta=10.0):
        super().__init__()
        mods = []
        for W, b in zip(Ws, bs):
            m = torch.nn.Linear(W.shape[1], W.shape[0])
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(W))
                m.bias.copy_(torch.from_numpy(b))
            mods += [m, torch.nn.Softplus(beta=beta)]
        self.net = torch.nn.Sequential(*mods)
        self.register_buffer("frequencies", torch.from_numpy(np.asarray(freqs, f32)))

    @torch.no_grad()
    def forward(self, x, double=False):
        """double: the same network in f64 on the same embedding ARGUMENTS (x * f is an f32 product by definition: at the
        high frequencies its rounding is many periods, an f64 product would be another function)."""
        embed = (x[..., None] * self.frequencies).view(*x.shape[:-1], -1)
        net = self.net
        if double:
            embed = embed.double()
            net = torch.nn.Sequential(*[torch.nn.Linear(m.in_features, m.out_features).double() if isinstance(m, torch.nn.Linear)
                                        else m for m in self.net])
            for a, b in zip(net, self.net):
                if isinstance(a, torch.nn.Linear):
                    a.weight.copy_(b.weight.double())
                    a.bias.copy_(b.bias.double())
        raw = net(torch.cat((embed.sin(), embed.cos()), dim=-1))
        return 1 - (-raw).exp()


def torch_march(rho, lengths, threshold, eps=1e-10):
    """pren.py:342-365 with thresholdMode (threshold >= 0) or plain emission-absorption, surface_thickness 1, and the
    callers' depth (genFeat.py:191-193): -> (weights, depth)."""
    rho = rho.clone()
    if threshold >= 0:
        c1 = rho * 0
        c1[torch.where(rho > threshold)] = 1
        rho = c1
    cp = torch.cumprod((1.0 + eps) - rho, dim=-1)
    absorption = torch.cat([torch.ones_like(cp[..., :1]), cp[..., :-1]], dim=-1)       # _shifted_cumprod, shift 1
    weights = rho * absorption
    return weights, torch.max(lengths * weights, dim=-1)[0]


def grid_points(res):
    """batched_forward_forPC's gridCoords (nerf.py:683-688), flat, and the index map of the two movedims of nerf.py:700."""
    t = np.linspace(-1, 1, res)
    pts = np.asarray([[z0, y0, x0] for x0 in t for y0 in t for z0 in t]).astype(f32)
    return pts


def record(section, entry):
    """Merge one measured pair into the parity record."""
    data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
    data.setdefault(section, {}).update(entry)
    PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
