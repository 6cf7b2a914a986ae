"""Shared by the contrastive-loss tests (not a test module): a NumPy restatement of include/isr_contrastive.h with every fmaf
chain and every sum order spelled out (vectorised over whatever the order leaves free), the reference formula in torch, input
makers, and the measured-margin record profiles/contrastive_parity.json."""
import json
from pathlib import Path

import numpy as np

from tests.density_ref import fma32, log1p64

ROOT = Path(__file__).resolve().parent.parent
PARITY = ROOT / "profiles" / "contrastive_parity.json"
PARITY_MARGIN = 4.0          # the project's standing bound: x the reference's own f32-to-f64 deviation
f32, f64 = np.float32, np.float64
BLOCK, SUPER, REDUCE = 64, 16, 256
NAN = np.array([0x7FC00000], np.uint32).view(f32)[0]


def canonical(x):
    x = np.asarray(x, f32)
    out = x.copy()
    out[np.isnan(x)] = NAN
    return out


def exp32(x):
    x = np.asarray(x, f32)
    nan, lo = np.isnan(x), x < f32(-87.0)
    xs = np.where(nan | lo, f32(0), x).astype(f32)
    kf = np.rint(xs * f32(1.44269504088896341)).astype(f32)
    r = fma32(kf, f32(-0.693359375), xs)
    r = fma32(kf, f32(2.12194440e-4), r)
    p = np.full(r.shape, f32(1.9875691500e-4), f32)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = fma32(p, r, f32(c))
    e = fma32(r * r, p, r) + f32(1.0)
    scale = ((kf.astype(np.int32) + 127) << 23).astype(np.int32).view(f32)
    return np.where(nan, NAN, np.where(lo, f32(0), e * scale)).astype(f32)


def logits(a, c):
    """dot(a_i, c_j) for a (R, D), c (C, D) -> (R, C): a_0 c_0, then fmaf(a_d, c_d, .) for d ascending."""
    with np.errstate(invalid="ignore", over="ignore"):
        l = (a[:, None, 0] * c[None, :, 0]).astype(f32)
        for d in range(1, a.shape[1]):
            l = fma32(a[:, None, d], c[None, :, d], l)
    return l


def row_dot(a, c):
    with np.errstate(invalid="ignore", over="ignore"):
        l = (a[:, 0] * c[:, 0]).astype(f32)
        for d in range(1, a.shape[1]):
            l = fma32(a[:, d], c[:, d], l)
    return l


def reduce_sum(v):
    """REDUCE ORDER over a 1-D f64 array."""
    v = np.asarray(v, f64)
    while True:
        L = -(-len(v) // REDUCE)
        w = np.zeros(L * REDUCE, f64)
        w[:len(v)] = v
        w = w.reshape(L, REDUCE).copy()
        s = REDUCE // 2
        while s:
            w[:, :s] += w[:, s:2 * s]
            s //= 2
        v = w[:, 0].copy()
        if L == 1:
            return v[0]


def _sets(q, n):
    """(rows of q as (R, D), the negatives they meet) per negative set."""
    B, S, D = q.shape
    if n.shape[0] == 1:
        return [(slice(0, B * S), n[0])]
    return [(slice(b * S, (b + 1) * S), n[b]) for b in range(B)]


def forward(q, k, n, scale):
    """-> m, t, pos, rows (B, S) and loss, by the rule."""
    B, S, D = q.shape
    qf, kf = q.reshape(-1, D), k.reshape(-1, D)
    pos = row_dot(qf, kf)
    m, t = np.empty(B * S, f32), np.empty(B * S, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, neg in _sets(q, n):
            L = logits(qf[rows], neg)
            mm = pos[rows].copy()
            for j in range(L.shape[1]):
                l = L[:, j]
                mm = np.where((l > mm) | np.isnan(l), l, mm)
            T = exp32(pos[rows] - mm).astype(f64)
            E = exp32(L - mm[:, None])
            for j0 in range(0, L.shape[1], BLOCK):
                c = np.zeros(L.shape[0], f32)
                for j in range(j0, min(j0 + BLOCK, L.shape[1])):
                    c = c + E[:, j]
                T = T + c.astype(f64)
            m[rows], t[rows] = mm, log1p64(T - 1.0).astype(f32)
        row = t - (pos - m)
        R = reduce_sum(canonical(row).astype(f64))
        loss = f32(f64(scale) * (R / f64(B * S)))
    shape = (B, S)
    return canonical(m).reshape(shape), canonical(t).reshape(shape), canonical(pos).reshape(shape), canonical(row).reshape(shape), canonical(loss)


def backward(q, k, n, scale, m, t, g=1.0):
    """-> dq, dk, dn by the rule."""
    B, S, D = q.shape
    qf, kf, m, t = q.reshape(-1, D), k.reshape(-1, D), m.reshape(-1), t.reshape(-1)
    c = f32((f64(f32(g)) * f64(scale)) / f64(B * S))
    with np.errstate(invalid="ignore", over="ignore"):
        a = exp32((row_dot(qf, kf) - m) - t) - f32(1.0)
        dk = (c * a)[:, None] * qf
        dq, dn = np.empty_like(qf), np.empty_like(n)
        for b, (rows, neg) in enumerate(_sets(q, n)):
            L = logits(qf[rows], neg)
            P = exp32((L - m[rows, None]) - t[rows, None])
            R, M = P.shape
            outer = np.zeros((R, D), f32)
            for j0 in range(0, M, BLOCK):
                inner = np.zeros((R, D), f32)
                for j in range(j0, min(j0 + BLOCK, M)):
                    inner = fma32(P[:, j, None], neg[None, j, :], inner)
                outer = outer + inner
            dq[rows] = c * fma32(a[rows, None], kf[rows], outer)
            qs = qf[rows]
            outer = np.zeros((M, D), f32)
            for s0 in range(0, R, BLOCK * SUPER):
                mid = np.zeros((M, D), f32)
                for i0 in range(s0, min(s0 + BLOCK * SUPER, R), BLOCK):
                    inner = np.zeros((M, D), f32)
                    for i in range(i0, min(i0 + BLOCK, R)):
                        inner = fma32(P[i, :, None], qs[None, i, :], inner)
                    mid = mid + inner
                outer = outer + mid
            dn[b] = c * outer
    return canonical(dq).reshape(q.shape), canonical(dk).reshape(q.shape), canonical(dn)


def inputs(rng, B, S, M, D, Bn, sigma=1.0):
    q, k = (rng.standard_normal((B, S, D)) * sigma).astype(f32), (rng.standard_normal((B, S, D)) * sigma).astype(f32)
    return q, k, (rng.standard_normal((Bn, M, D)) * sigma).astype(f32)


TREE_EDGES = (1, 256, 257, 65536, 65537)                  # REDUCE ORDER's level edges: one tree, two levels, three


def tree_edge_inputs(rows):
    """q, k, n of B S = rows rows with M = 1 and D = 4: the loss is a sum over `rows` leaves and little else."""
    return inputs(np.random.default_rng(20261022 + rows), 1, rows, 1, 4, 1)


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == f32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def torch_loss(q, k, n, scale=None):
    """The reference's formula (nutil.py:368-385) in torch, on q's device and in q's dtype; n (1, M, D) is expanded.  scale
    None: the reference's own / 1000."""
    import torch
    from torch.nn import functional as F
    sim_pos = (k * q).sum(dim=-1, keepdim=True)
    sim_neg = q @ n.expand(q.shape[0], -1, -1).permute(0, 2, 1)
    lgts = torch.cat((sim_pos, sim_neg), dim=-1).permute(0, 2, 1)
    target = torch.zeros(sim_pos.shape[0], sim_pos.shape[1], dtype=torch.long, device=q.device)
    ce = F.cross_entropy(lgts, target)
    return ce / 1000 if scale is None else ce * scale


def ulp32(x) -> float:
    return float(np.spacing(np.abs(f32(x))))


def record(section: str, values: dict) -> None:
    """Merge measured ratios into profiles/contrastive_parity.json (only when ISR_RECORD_PARITY is set: tests do not write)."""
    import os
    if not os.environ.get("ISR_RECORD_PARITY"):
        return
    data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
    data.setdefault(section, {}).update(values)
    PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
