"""Shared by the tests of the sampling's backward (not a test module): a NumPy restatement of include/isr_sample_grad.h — a
plain double loop over images and rays with f32 additions, over a restatement of csrc/rays.hpp's nearest_pixel — the f64
sums the bound against torch needs, and the cases the CPU and the GPU tests share."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def nearest_pixel(v, size: int):
    """rays.hpp's nearest_pixel, every operation rounded to f32: rint(((-v + 1) / 2) * (size - 1)), half to even; -1 outside
    0 .. size - 1 and for NaN."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.rint(((-v + f32(1)) / f32(2)) * f32(size - 1))
        ok = (f >= 0) & (f <= f32(size - 1))
    return np.where(ok, np.where(ok, f, 0), -1).astype(np.int64)


def backward_ref(dout, xys, H: int, W: int):
    """dout (B, n, C), xys (B, n, 2) -> dimages (B, H, W, C): r ascending, acc = acc + dout in f32 from +0."""
    dout, xys = np.asarray(dout, f32), np.asarray(xys, f32)
    B, n, C = dout.shape
    ix, iy = nearest_pixel(xys[..., 0], W), nearest_pixel(xys[..., 1], H)
    out = np.zeros((B, H, W, C), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for r in range(n):
                if ix[b, r] >= 0 and iy[b, r] >= 0:
                    out[b, iy[b, r], ix[b, r]] = out[b, iy[b, r], ix[b, r]] + dout[b, r]
    return out


def sums_f64(dout, xys, H: int, W: int):
    """-> (sum of dout, sum of |dout|) per (pixel, channel) in f64, (B, H, W, C) each, and the ray count m (B, H, W)."""
    dout, xys = np.asarray(dout, f32), np.asarray(xys, f32)
    B, n, C = dout.shape
    ix, iy = nearest_pixel(xys[..., 0], W), nearest_pixel(xys[..., 1], H)
    s, a, m = np.zeros((B, H, W, C)), np.zeros((B, H, W, C)), np.zeros((B, H, W), np.int64)
    keep = (ix >= 0) & (iy >= 0)
    b = np.broadcast_to(np.arange(B)[:, None], (B, n))[keep]
    np.add.at(s, (b, iy[keep], ix[keep]), dout[keep].astype(np.float64))
    np.add.at(a, (b, iy[keep], ix[keep]), np.abs(dout[keep].astype(np.float64)))
    np.add.at(m, (b, iy[keep], ix[keep]), 1)
    return s, a, m


def chain_bound(a, m):
    """(m - 1) * 2^-24 * sum|dout|: the first-order bound of a chain of m - 1 f32 additions; 0 where m <= 1."""
    return np.maximum(m - 1, 0)[..., None] * 2.0 ** -24 * a


def at_pixel(i, size: int):
    """The NDC coordinate whose nearest pixel is i (i may be fractional) on an axis of `size` pixels."""
    i = np.asarray(i, np.float64)
    return (-(2.0 * i / (size - 1) - 1.0) if size > 1 else np.zeros_like(i)).astype(f32)


def on_pixels(iy, ix, H: int, W: int):
    """xys (n, 2) of rays at the pixels (iy[k], ix[k])."""
    return np.stack([at_pixel(ix, W), at_pixel(iy, H)], -1)


def random_case(rng, B: int, H: int, W: int, C: int, n: int, spread: float = 1.1):
    return (rng.standard_normal((B, n, C)).astype(f32), rng.uniform(-spread, spread, (B, n, 2)).astype(f32), H, W)


def one_pixel_case(rng, B: int, H: int, W: int, C: int, n: int):
    xy = np.broadcast_to(on_pixels([H // 2], [W // 3], H, W), (B, n, 2)).copy()
    return rng.standard_normal((B, n, C)).astype(f32), xy, H, W


def cases():
    """name -> (dout (B, n, C), xys (B, n, 2), H, W): the edge cases of the issue, small enough for the double loop."""
    rng = np.random.default_rng(20240521)
    out = {"n = 1": random_case(rng, 2, 4, 5, 3, 1, spread=0.9)}
    for n in (2, 64, 65, 4097):
        out[f"every ray on one pixel, n = {n}"] = one_pixel_case(rng, 1 if n > 65 else 2, 5, 7, 3, n)
    iy, ix = np.divmod(np.arange(15), 5)
    out["every ray on its own pixel, 3 x 5"] = (rng.standard_normal((1, 15, 2)).astype(f32), on_pixels(iy, ix, 3, 5)[None], 3, 5)
    xy = np.array([[1.5, 0], [-1.5, 0], [0, 1.5], [0, -1.5], [np.nan, 0], [0, np.nan], [np.inf, 0], [0, -np.inf], [0.2, -0.3],
                   [1.0, 1.0], [-1.0, -1.0], [np.nan, np.nan]], f32)
    out["outside on each side, NaN and infinite coordinates"] = (rng.standard_normal((1, len(xy), 2)).astype(f32), xy[None], 4, 6)
    half = np.arange(0.5, 4, 1.0)                      # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4 on 5 pixels: exact in f32
    xy = np.stack([np.concatenate([at_pixel(half, 5), at_pixel([1, 3], 5)]), np.concatenate([at_pixel([0, 1, 2, 3], 5), at_pixel([1.5, 2.5], 5)])], -1)
    out["exact half-integer positions"] = (rng.standard_normal((1, 6, 2)).astype(f32), xy[None], 5, 5)
    out["W = 1"] = random_case(rng, 2, 6, 1, 2, 40)
    out["H = 1"] = random_case(rng, 2, 1, 6, 2, 40)
    out["H = W = 1"] = random_case(rng, 1, 1, 1, 2, 9)
    for C in (1, 12, 13, 65):
        out[f"C = {C}"] = random_case(rng, 2, 6, 7, C, 100)
    d, xy, H, W = random_case(rng, 3, 5, 6, 4, 50)
    xy[1] = 1.5
    out["B = 3, the middle image keeps nothing"] = (d, xy, H, W)
    d, xy, H, W = random_case(rng, 2, 4, 4, 3, 60)
    out["dout of zeros"] = (np.zeros_like(d), xy, H, W)
    out["dout of -0"] = (np.full_like(d, -0.0), xy, H, W)
    d = d.copy()
    d[0, 7, 1], d[1, 11, 2] = np.nan, np.inf
    out["dout with a NaN and an infinity"] = (d, xy, H, W)
    return out


def same_bits(a, b) -> bool:
    """Bit equality of two f32 arrays, -0 and +0 apart; a NaN equals a NaN (its payload is the adder's business)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[keep], b.view(np.uint32)[keep])
