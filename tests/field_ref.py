"""Shared by the key-field tests (not a test module): SIREN-initialised fields, their f64 NumPy evaluation, the same layers
as a torch module, and the measured-margin record profiles/key_field_parity.json."""
import json
from pathlib import Path

import numpy as np
import torch

PARITY = Path(__file__).resolve().parent.parent / "profiles" / "key_field_parity.json"


def siren_params(widths, omegas, seed=0):
    """Sitzmann et al. 2020, sec. 3.2: first layer U(-1/in, 1/in), the others U(-sqrt(6/in)/omega, sqrt(6/in)/omega) (omega 30
    for a linear last layer); biases torch.nn.Linear's U(-1/sqrt(in), 1/sqrt(in)).  f32 arrays."""
    rng = np.random.default_rng(seed)
    Ws, bs = [], []
    for l, (i, o) in enumerate(zip(widths[:-1], widths[1:])):
        lim = 1.0 / i if l == 0 else np.sqrt(6.0 / i) / (omegas[l] if omegas[l] is not None else 30.0)
        Ws.append(rng.uniform(-lim, lim, (o, i)).astype(np.float32))
        bs.append(rng.uniform(-1, 1, o).astype(np.float32) / np.float32(np.sqrt(i)))
    return Ws, bs


def eval_f64(Ws, bs, omegas, pts):
    h = np.asarray(pts, np.float32).astype(np.float64)
    for W, b, om in zip(Ws, bs, omegas):
        z = h @ W.astype(np.float64).T + b.astype(np.float64)
        h = z if om is None else np.sin(np.float64(np.float32(om)) * z)
    return h


class TorchField(torch.nn.Module):
    """The same layers as framework calls, and driven as the reference drives its field (nerf.py:404-457)."""

    def __init__(self, Ws, bs, omegas):
        super().__init__()
        self.linears = torch.nn.ModuleList()
        for W, b in zip(Ws, bs):
            m = torch.nn.Linear(W.shape[1], W.shape[0])
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(W))
                m.bias.copy_(torch.from_numpy(b))
            self.linears.append(m)
        self.omegas = list(omegas)

    @torch.no_grad()
    def forward(self, x):
        for m, om in zip(self.linears, self.omegas):
            x = m(x)
            if om is not None:
                x = torch.sin(om * x)
        return x

    @torch.no_grad()
    def batched_customForward(self, x, n_batches=16):
        parts = [self.forward(c) for c in torch.chunk(x, n_batches)]
        f = torch.cat(parts)
        return torch.cat([f, torch.zeros(len(f), 1, device=f.device)], dim=-1)


def record(section, entry):
    """Merge one measured pair into the parity record."""
    data = json.loads(PARITY.read_text()) if PARITY.exists() else {}
    data.setdefault(section, {}).update(entry)
    PARITY.write_text(json.dumps(data, indent=1, sort_keys=True) + "\n")
