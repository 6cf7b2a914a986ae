"""Shared by the key-field backward tests (not a test module): a NumPy restatement of include/isr_field_grad.h with every fmaf
and every rounding where the header puts it (fma32 of tests/density_ref.py; sin32 / cos32 restated in f64), the fields and
upstream cases the tests run, the same gradients by torch autograd, and the record profiles/field_grad_parity.json."""
import json
import os
from pathlib import Path

import numpy as np
import torch

from tests import field_ref
from tests.density_ref import fma32

ROOT = Path(__file__).resolve().parent.parent
PARITY = ROOT / "profiles" / "field_grad_parity.json"
PARITY_MARGIN = 4.0                     # the project's standing rule for "inside the reference's own rounding"
f32, f64 = np.float32, np.float64

# name -> (widths, omegas): one layer; a padded hidden layer; three matrix-core layers of odd widths; the reference's head;
# a linear hidden layer; a narrow layer above layer 0 (the vector path of the u pass) under a linear last layer
FIELDS = {
    "3-12": ((3, 12), (30.0,)),
    "3-32-12": ((3, 32, 12), (30.0, 30.0)),
    "3-40-33-5": ((3, 40, 33, 5), (30.0, 1.5, 2.0)),
    "3-256-256-256-12": ((3, 256, 256, 256, 12), (30.0, 30.0, 30.0, 30.0)),
    "linear hidden": ((3, 40, 33, 7), (30.0, None, 2.0)),
    "narrow second": ((3, 5, 40, 7), (30.0, 1.5, None)),
}
UPSTREAMS = ("ones", "random", "zero", "one row")


def field(name, seed=0):
    """-> (widths, omegas, Ws, bs) with SIREN-initialised weights."""
    widths, omegas = FIELDS[name]
    Ws, bs = field_ref.siren_params(widths, omegas, seed=seed)
    return widths, omegas, Ws, bs


def inputs(widths, N, upstream="random", seed=0, ld=None):
    rng = np.random.default_rng(seed * 1000003 + N)
    pts = rng.uniform(-1, 1, (N, 3)).astype(f32)
    ld = widths[-1] if ld is None else ld
    dout = rng.normal(size=(N, ld)).astype(f32)
    if upstream == "ones":
        dout[:] = 1
    elif upstream == "zero":
        dout[:] = 0
    elif upstream == "one row":
        keep = dout[N // 2].copy() if N else None
        dout[:] = 0
        if N:
            dout[N // 2] = keep
    return pts, dout


def sincos32(a):
    """sin32 and cos32 of csrc/field_mlp.hpp / csrc/field_grad.hpp on an f32 array, operation for operation in f64."""
    x = np.asarray(a, f32).astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.rint(x * 6.36619772367581382433e-01)
        r0 = (x - n * 1.57079632673412561417e+00) - n * 6.07710050650619224932e-11
        r = np.where(n == 0.0, x, r0)
        r = np.where(r > 1.0, 1.0, np.where(r < -1.0, -1.0, r))
        r2 = r * r
        ps = -1.66666666666666324348e-01 + r2 * (8.33333333332248946124e-03 + r2 * (-1.98412698298579493134e-04 + r2 * (
            2.75573137070700676789e-06 + r2 * (-2.50507602534068634195e-08 + r2 * 1.58969099521155010221e-10))))
        pc = -0.5 + r2 * (4.16666666666666019037e-02 + r2 * (-1.38888888888741095749e-03 + r2 * (2.48015872894767294178e-05 + r2 * (
            -2.75573143513906633035e-07 + r2 * (2.08757232129817482790e-09 + r2 * -1.13596475577881948265e-11)))))
        s = r * (1.0 + r2 * ps)
        c = 1.0 + r2 * pc
        q = n - 4.0 * np.rint(n * 0.25)
        sn = np.where(q == 0.0, s, np.where(q == 1.0, c, np.where(q == -1.0, -c, -s)))
        cs = np.where(q == 0.0, c, np.where(q == 1.0, -s, np.where(q == -1.0, s, -c)))
        return sn.astype(f32), cs.astype(f32)


def blocked(g, h, chain):
    """sum_n g[n, :, None] * h[n, None, :] in the rule's order: f32 chains over blocks of `chain` points, the block sums added
    in f64 in block order, one rounding to f32."""
    total = np.zeros((g.shape[1], h.shape[1]), f64)
    for n0 in range(0, g.shape[0], chain):
        acc = np.zeros(total.shape, f32)
        for n in range(n0, min(n0 + chain, g.shape[0])):
            acc = fma32(g[n, :, None], h[n, None, :], acc)
        with np.errstate(invalid="ignore"):
            total = total + acc.astype(f64)
    return total.astype(f32)


def backward(Ws, bs, omegas, pts, dout, chain):
    """-> (dW, db) flat in the standard layout, by the rule of include/isr_field_grad.h."""
    N = pts.shape[0]
    h, H, S = np.asarray(pts, f32), [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for W, b, om in zip(Ws, bs, omegas):
            H.append(h)
            z = np.broadcast_to(b.astype(f32), (N, W.shape[0])).copy()
            for k in range(W.shape[1]):
                z = fma32(W[None, :, k], h[:, k, None], z)
            if om is None:
                h = z
                S.append(None)
            else:
                sn, cs = sincos32(f32(om) * z)
                h = sn
                S.append(f32(om) * cs)
        u = np.ascontiguousarray(dout[:, :Ws[-1].shape[0]], f32)
        dW, db = [None] * len(Ws), [None] * len(Ws)
        for l in range(len(Ws) - 1, -1, -1):
            g = u if S[l] is None else u * S[l]
            dW[l] = blocked(g, H[l], chain).reshape(-1)
            db[l] = blocked(g, np.ones((N, 1), f32), chain).reshape(-1)
            if l:
                acc = np.zeros((N, Ws[l].shape[1]), f32)
                for j in range(Ws[l].shape[0]):
                    acc = fma32(Ws[l][None, j, :], g[:, j, None], acc)
                u = acc
    return np.concatenate(dW), np.concatenate(db)


def pack_t(widths, Ws):
    """The transposed pack of include/isr_field_grad.h restated: 64 zero words, then per layer l >= 1 W_l^T as a layer with
    in = out_l rounded up to 32 in matrix-core order (in_l >= 32), or in = out_l rounded up to 4 row-major, out = in_l rounded
    up to 32, and a zero bias; everything else zero."""
    parts = [np.zeros(64, f32)]
    for K, O, W in list(zip(widths[:-1], widths[1:], Ws))[1:]:
        mfma = K >= 32
        kin = (O + 31) // 32 * 32 if mfma else O
        ks = (kin + 7) // 8 * 8 if mfma else (kin + 3) // 4 * 4
        OPt = (K + 31) // 32 * 32
        block = np.zeros(OPt * ks + OPt, f32)
        j, k = np.meshgrid(np.arange(K), np.arange(O), indexing="ij")          # the transposed layer's neuron j is W's input
        lane = (k & 1) * 32 + (j & 31)
        idx = ((((j >> 5) * (ks >> 3) + (k >> 3)) * 64 + lane) * 4 + ((k & 7) >> 1)) if mfma else j * ks + k
        block[idx] = W.T
        parts.append(block)
    return np.concatenate(parts)


def same(a, b) -> bool:
    """Bit equality with NaN-aware comparison: NaNs in the same places, every other entry the same bits."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def torch_grads(Ws, bs, omegas, pts, dout, dtype, device="cpu", chunks=1):
    """The same layers as torch.nn.Linear modules (field_ref.TorchField) under torch autograd in `dtype`, the loss
    sum(out * dout) -> per layer (dW_l, db_l) as f64 NumPy arrays."""
    tf = field_ref.TorchField(Ws, bs, omegas).to(device=device, dtype=dtype)
    x = torch.from_numpy(np.ascontiguousarray(pts)).to(device=device, dtype=dtype)
    up = torch.from_numpy(np.ascontiguousarray(dout[:, :Ws[-1].shape[0]])).to(device=device, dtype=dtype)
    for xc, uc in zip(torch.chunk(x, chunks), torch.chunk(up, chunks)):
        for m, om in zip(tf.linears, tf.omegas):
            xc = m(xc)
            if om is not None:
                xc = torch.sin(om * xc)
        (xc * uc).sum().backward()
    return [(m.weight.grad.double().cpu().numpy(), m.bias.grad.double().cpu().numpy()) for m in tf.linears]


def split(widths, dW, db):
    """Flat standard-layout gradients -> per layer (dW_l (out, in), db_l)."""
    out, wo, bo = [], 0, 0
    for i, o in zip(widths[:-1], widths[1:]):
        out.append((dW[wo:wo + o * i].reshape(o, i), db[bo:bo + o]))
        wo, bo = wo + o * i, bo + o
    return out


def ulp32(x) -> float:
    return float(np.spacing(f32(abs(x))))


def within_margin(tag, widths, ours, r32, r64, record_section=None):
    """Every dW_l and db_l of `ours` within PARITY_MARGIN x torch-f32's own largest deviation from f64 on that array (one f32
    ulp of the array's largest magnitude where torch's deviation is 0).  Prints and optionally records the multiples."""
    ok, entry = True, {}
    for l, (mine, a32, a64) in enumerate(zip(split(widths, *ours), r32, r64)):
        for name, x, y32, y64 in (("dW", mine[0], a32[0], a64[0]), ("db", mine[1], a32[1], a64[1])):
            e = float(np.abs(y32 - y64).max())
            dev = float(np.abs(x.astype(f64) - y64).max())
            bound = PARITY_MARGIN * e if e > 0 else ulp32(np.abs(y64).max())
            print(f"{tag}: {name}_{l} deviation {dev:.3e}, torch f32 {e:.3e}, multiple {dev / e if e > 0 else float('nan'):.2f}")
            entry[f"{name}_{l}"] = {"deviation": dev, "torch_f32": e, "multiple": dev / e if e > 0 else None}
            ok = ok and dev <= bound
    if record_section is not None and os.environ.get("ISR_RECORD_PARITY"):      # tests do not write unless asked to
        data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
        data.setdefault(record_section, {})[tag] = entry
        PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
    return ok
