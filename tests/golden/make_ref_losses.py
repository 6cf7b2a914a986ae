#!/usr/bin/env python3
"""Generates ref_contrastive.npz: the fixture that pins the contrastive key loss to the reference's EXECUTED code.

  returnCrossEntropy         nutil.py:349-366
  returnCrossEntropyWithNeg  nutil.py:368-385
  returnCrossEntropy2        nutil.py:386-403

As make_ref_resample.py does: nothing of the reference is imported or stored, each function is parsed with `ast`, compiled
and executed with device="cpu" under torch autograd, and only DATA is written.  Every case runs in f32 and, with the same
inputs widened, in f64.  Stored per case: the inputs (f32), the f64 loss and gradients (what the tests compare with), the f32
loss, and for the loss and each gradient array the largest deviation of the f32 run from the f64 run (`*_eref`: what the
tests' tolerance is measured from).  The f32 gradient arrays themselves are not stored (they are as large as the f64 ones).

Cases.  returnCrossEntropyWithNeg: inputs N(0, 1) scaled by 0.3, 1 and 3 at (B, S, M, D) = (2, 65, 130, 12); scaled by 1 at
(1, 96, 257, 12) and (2, 64, 1024, 12); (2, 40, 130, 32).  returnCrossEntropy (B = 1: its target tensor admits nothing else):
(1, 65, 12) with negFrac 0.5 and (1, 130, 12) with negFrac 1, the host generator seeded with SEED before each call and the
drawn negKeys recorded.  returnCrossEntropy2: (1, 96, 12) with 40 recorded negKeys.

Run from the repo root:  python tests/golden/make_ref_losses.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
from make_golden_from_reference import ref_function                                                      # noqa: E402
from make_ref_fields import _save                                                                        # noqa: E402

f32, f64 = np.float32, np.float64
SEED = 20261019
WITH_NEG = {"a03": (2, 65, 130, 12, 0.3), "a1": (2, 65, 130, 12, 1.0), "a3": (2, 65, 130, 12, 3.0), "b1": (1, 96, 257, 12, 1.0),
            "c1": (2, 64, 1024, 12, 1.0), "d32": (2, 40, 130, 32, 1.0)}
OWN_KEYS = {"e05": (1, 65, 12, 0.5), "e1": (1, 130, 12, 1.0)}


def run(fn, arrays, dtype, **kw):
    """fn(*arrays as leaf tensors, device='cpu', **kw) -> (loss, gradients) as NumPy."""
    ts = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in arrays]
    loss = fn(*ts, device="cpu", **kw)
    loss.backward()
    return loss.detach().numpy(), [t.grad.numpy() for t in ts]


def store(out, tag, fn, arrays, names, **kw):
    l32, g32 = run(fn, arrays, torch.float32, **kw)
    l64, g64 = run(fn, arrays, torch.float64, **kw)
    assert l32.dtype == f32 and l64.dtype == f64
    out[f"{tag}_loss_f32"], out[f"{tag}_loss_f64"] = l32, l64
    out[f"{tag}_loss_eref"] = np.array(abs(f64(l32) - l64))
    for name, a, b in zip(names, g32, g64):
        out[f"{tag}_d{name}_f64"] = b
        out[f"{tag}_d{name}_eref"] = np.array(np.abs(a.astype(f64) - b).max())
        assert out[f"{tag}_d{name}_eref"] > 0, f"{tag}: the f32 d{name} equals the f64 one: no tolerance to measure"
    for name, a in zip(names, arrays):
        out[f"{tag}_{name}"] = a


def main():
    ns = {"torch": torch}
    with_neg = ref_function("nutil.py", "returnCrossEntropyWithNeg", ns)
    own = ref_function("nutil.py", "returnCrossEntropy", ns)
    own2 = ref_function("nutil.py", "returnCrossEntropy2", ns)
    rng = np.random.default_rng(SEED)
    out = {"seed": np.array([SEED], np.int64)}
    for tag, (B, S, M, D, sigma) in WITH_NEG.items():
        q, k, n = ((rng.standard_normal(shape) * sigma).astype(f32) for shape in ((B, S, D), (B, S, D), (B, M, D)))
        store(out, tag, with_neg, (q, k, n), "qkn")
    for tag, (B, S, D, frac) in OWN_KEYS.items():
        q, k = (rng.standard_normal((B, S, D)).astype(f32) for _ in range(2))
        torch.manual_seed(SEED)
        out[f"{tag}_negKeys"] = torch.randperm(S, dtype=torch.int64)[0: int(S * frac)].numpy()
        torch.manual_seed(SEED)                                    # the same draw in both runs
        l32, g32 = run(own, (q, k), torch.float32, negFrac=frac)
        torch.manual_seed(SEED)
        l64, g64 = run(own, (q, k), torch.float64, negFrac=frac)
        out[f"{tag}_negFrac"] = np.array([frac], f64)
        out[f"{tag}_loss_f32"], out[f"{tag}_loss_f64"], out[f"{tag}_loss_eref"] = l32, l64, np.array(abs(f64(l32) - l64))
        for name, a, b, x in zip("qk", g32, g64, (q, k)):
            out[f"{tag}_d{name}_f64"], out[f"{tag}_d{name}_eref"], out[f"{tag}_{name}"] = b, np.array(np.abs(a.astype(f64) - b).max()), x
    q, k = (rng.standard_normal((1, 96, 12)).astype(f32) for _ in range(2))
    keys = torch.from_numpy(rng.permutation(96)[:40].astype(np.int64))
    out["f2_negKeys"] = keys.numpy()
    store(out, "f2", own2, (q, k), "qk", negKeys=keys)
    _save("ref_contrastive.npz", out)


if __name__ == "__main__":
    main()
