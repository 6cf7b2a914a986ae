"""NumPy restatement of include/isr_adam.h (test infrastructure): the scalars of a step in f64 (Python floats, the f64 fma
of the paired powering by exact rational arithmetic), the elements in np.float32, every fmaf of the header as the exact
product in f64, one f64 addition rounded to odd, and one rounding to f32 — which is fmaf's single rounding (an f32 product
is exact in f64, and 53 bits rounded to odd leave the rounding to 24 bits what it would have been from the exact sum)."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64
CHUNK = 4096
SIZES = (0, 1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7)      # the element counts every test mixes


def fma64(a: float, b: float, c: float) -> float:
    """fma in f64, one rounding (finite arguments)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def dd_mul(ah, al, ch, cl):
    p = ah * ch
    e = fma64(ah, ch, -p)
    e = fma64(ah, cl, e)
    e = fma64(al, ch, e)
    h = p + e
    return h, e - (h - p)


def pow_int(beta: float, t: int) -> float:
    rh, rl, bh, bl = 1.0, 0.0, float(beta), 0.0
    while t > 0:
        if t & 1:
            rh, rl = dd_mul(rh, rl, bh, bl)
        t >>= 1
        if t > 0:
            bh, bl = dd_mul(bh, bl, bh, bl)
    return rh


def lr_at(lr: float, ramp: float, t: int) -> float:
    if not ramp > 0:
        return lr
    frac = float(t + 1) / ramp
    return lr * (frac if frac < 1.0 else 1.0)


def scalars(group, t: int):
    """group = (lr, beta1, beta2, eps, weight_decay, ramp), t the 1-based step -> (step, r) as np.float32."""
    lr, b1, b2, _, _, ramp = (float(x) for x in group)
    bc1, bc2 = 1.0 - pow_int(b1, t), 1.0 - pow_int(b2, t)
    with np.errstate(all="ignore"):
        return f32(f64(lr_at(lr, ramp, t)) / f64(bc1)), f32(math.sqrt(bc2))


def fmaf(a, b, c):
    """fmaf over np.float32 arrays (or scalars): a * b + c with one rounding."""
    a, b, c = (np.asarray(x, f32).astype(f64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        x = a * b                                                                     # exact: 48 bits
        s = x + c
        bb = s - x
        err = (x - (s - bb)) + (c - bb)                                               # two-sum: s + err = x + c exactly
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (s.view(np.int64) & 1) == 0
        odd = np.where(inexact & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)      # the neighbour on err's side
        return odd.astype(f32)


def update(group, t: int, p, g, m, v):
    """One step of one tensor (np.float32 arrays of one shape) -> (p', m', v')."""
    _, b1, b2, eps, wd, _ = (float(x) for x in group)
    step, r = scalars(group, t)
    c1, c2, b2f, epsf, wdf = f32(1.0 - b1), f32(1.0 - b2), f32(b2), f32(eps), f32(wd)
    with np.errstate(all="ignore"):
        g1 = fmaf(wdf, p, g) if wdf != 0 else g.astype(f32)
        m1 = fmaf(c1, (g1 - m).astype(f32), m)
        v1 = fmaf(c2, (g1 * g1).astype(f32), (b2f * v).astype(f32))
        denom = ((np.sqrt(v1).astype(f32) / r).astype(f32) + epsf).astype(f32)
        p1 = fmaf(-step, (m1 / denom).astype(f32), p)
    return p1, m1, v1


def step(params, grads, exp_avgs, exp_avg_sqs, group_of, groups, steps, slots=None, zero_grads=False) -> None:
    """ops.adam_step_host's arguments and effect: in place over lists of float32 arrays, steps int64."""
    slots = list(range(len(params))) if slots is None else list(slots)
    for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        p1, m1, v1 = update(groups[group_of[i]], int(steps[slots[i]]) + 1, p, g, m, v)
        p[...], m[...], v[...] = p1, m1, v1
        if zero_grads:
            g[...] = 0
    for s in slots:
        steps[s] += 1


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_tensors(sizes, seed: int, g_lo: float = 1e-6, g_hi: float = 10.0, offsets=None):
    """Lists p, g, m, v of float32 arrays of the given sizes: parameters in [-1, 1], gradients of either sign with magnitudes
    log-uniform in [g_lo, g_hi], moments as after some steps (v >= 0).  offsets (per tensor, in elements, or None): each array is
    a view that far into a 16-byte-aligned buffer."""
    rng = np.random.default_rng(seed)
    out = ([], [], [], [])
    for i, n in enumerate(sizes):
        mag = np.exp(rng.uniform(np.log(g_lo), np.log(g_hi), n))
        vals = (rng.uniform(-1, 1, n), mag * rng.choice([-1.0, 1.0], n), 0.1 * mag * rng.uniform(-1, 1, n),
                (mag * rng.uniform(0, 1, n)) ** 2)
        for lst, a in zip(out, vals):
            off = 0 if offsets is None else offsets[i]
            buf = aligned(n + off + 4)
            view = buf[off:off + n]
            view[...] = a.astype(f32)
            lst.append(view)
    return out


def aligned(n: int) -> np.ndarray:
    """n float32 at a 16-byte-aligned address."""
    raw = np.zeros(4 * n + 16, np.uint8)
    skip = (-raw.ctypes.data) % 16
    return raw[skip:skip + 4 * n].view(f32)


def clone(lists):
    """A copy of make_tensors' result with the same misalignments."""
    out = []
    for lst in lists:
        new = []
        for a in lst:
            off = (a.ctypes.data % 16) // 4
            b = aligned(a.size + off + 4)[off:off + a.size]
            b[...] = a
            new.append(b)
        out.append(new)
    return tuple(out)
