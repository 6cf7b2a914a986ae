"""Poisoned allocations (test infrastructure, not a conftest): every tensor made through torch.empty, torch.empty_like,
torch.empty_strided or Tensor.new_empty inside `poisoned(...)` is filled with one byte before it is returned — its whole
storage, whatever its strides — device tensors on the current stream, host tensors on the host.  An output a kernel forgets to write then holds that byte instead of whatever the
caching allocator handed back (usually the previous call's answer, or zeros).

    0xFF: NaN for f32 / f64 / bf16, -1 for signed integers.
    0x7F: 3.39e38 for f32, a large positive integer: catches an output used as the starting value of an atomicMax /
          atomicAdd.

torch.zeros / torch.full are left alone: the pre-fills some wrappers still make are part of their contracts.
ops.clear_workspaces() runs on entry and on exit, so the cached scratch is drawn from the poisoned allocator and no
poisoned buffer outlives the block."""
from __future__ import annotations

import contextlib
import dataclasses

import torch

BYTES = (0xFF, 0x7F)


def _fill(t, byte: int):
    """Every byte of t's storage (strided, offset or 0-d views included) set to `byte`."""
    store = t.untyped_storage()
    if store.nbytes():
        torch.tensor([], dtype=torch.uint8, device=t.device).set_(store).fill_(byte)
    return t


@contextlib.contextmanager
def poisoned(monkeypatch, byte: int):
    """Inside the block, torch.empty / empty_like / empty_strided / Tensor.new_empty return tensors filled with `byte`."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    empty, empty_like, empty_strided = torch.empty, torch.empty_like, torch.empty_strided
    new_empty = torch.Tensor.new_empty
    ops.clear_workspaces()
    try:
        with monkeypatch.context() as mp:
            mp.setattr(torch, "empty", lambda *a, **k: _fill(empty(*a, **k), byte))
            mp.setattr(torch, "empty_like", lambda *a, **k: _fill(empty_like(*a, **k), byte))
            mp.setattr(torch, "empty_strided", lambda *a, **k: _fill(empty_strided(*a, **k), byte))
            mp.setattr(torch.Tensor, "new_empty", lambda self, *a, **k: _fill(new_empty(self, *a, **k), byte))
            yield
            torch.cuda.synchronize()
    finally:
        ops.clear_workspaces()


def to_host(x):
    """Host copies of every tensor in a (nested) result: tuples, lists, dicts, dataclasses."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().clone()
    if dataclasses.is_dataclass(x) and not isinstance(x, type):
        return {f.name: to_host(getattr(x, f.name)) for f in dataclasses.fields(x)}
    if isinstance(x, dict):
        return {k: to_host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(to_host(v) for v in x) if isinstance(x, list) else tuple(to_host(v) for v in x)
    return x


def run_twice(monkeypatch, fn):
    """fn() once under 0xFF and once under 0x7F, synchronised; -> (result under 0xFF, result under 0x7F) as host copies."""
    out = []
    for byte in BYTES:
        with poisoned(monkeypatch, byte):
            r = fn()
            torch.cuda.synchronize()
            out.append(to_host(r))
    return out[0], out[1]


def bits(t: torch.Tensor) -> torch.Tensor:
    """The bytes of a host tensor (NaN-safe, -0.0-safe comparison)."""
    t = t.contiguous()
    if t.numel() == 0:
        return torch.zeros(0, dtype=torch.uint8)
    return (t.reshape(-1) if t.dim() == 0 else t).view(torch.uint8).reshape(-1)


def same_bits(a, b) -> bool:
    """Bit equality of two (nested) results of to_host."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return a == b
