"""Tensor-level wrappers over the C ABI: allocate outputs / workspace with torch (plumbing only)
and enqueue the HIP kernels on torch's current stream.  No arithmetic happens here."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

import torch

from . import _capi
from ._capi import check, current_stream, lib, ptr, require_cuda

_workspaces: dict[tuple, torch.Tensor] = {}

# Optional per-entry-point HIP-event timing (bench.py's live roofline measurement): when enabled,
# every wrapper brackets its C-ABI call with events on the stream it launches on and records
# (start, end, algorithmic work).  Off by default: no events, no overhead.
_timers: dict[str, list] | None = None


def enable_timing(on: bool = True) -> None:
    global _timers
    _timers = {} if on else None


def drain_timing() -> dict[str, tuple[int, float, float]]:
    """-> {name: (calls, total_ms, total_work)}; synchronises.  Clears the records."""
    out = {}
    if _timers is None:
        return out
    torch.cuda.synchronize()
    for name, recs in _timers.items():
        ms = sum(a.elapsed_time(b) for a, b, _ in recs)
        out[name] = (len(recs), ms, float(sum(w for _, _, w in recs)))
    _timers.clear()
    return out


class _timed:
    def __init__(self, name: str, work: float):
        self.name, self.work = name, work

    def __enter__(self):
        if _timers is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if _timers is not None:
            self.e1.record()
            _timers.setdefault(self.name, []).append((self.e0, self.e1, self.work))
        return False


class tuning:
    """Context manager over the library's tuning knobs (isr_tuning_set; experiments and tests only):
        with ops.tuning(nn_path=0): ...      # brute-force NN inside the block
    Knobs: nn_path (-1 auto, 0 brute, 1 per-lane grid, 2 block-cooperative grid), nn_filter (-1 auto, 0, 1),
    icp_warm (1, 0), nn_plan_rq, nn_plan_blocks, nn_tile_st / nn_tile_sq (x 1000), nn_tile_tb.  Process-wide:
    do not flip a knob while another thread is inside an entry point that reads it."""

    def __init__(self, **knobs):
        self.knobs = {_capi.TUNE[k]: int(v) for k, v in knobs.items()}

    def __enter__(self):
        L = lib()
        self.old = {k: L.isr_tuning_get(k) for k in self.knobs}
        for k, v in self.knobs.items():
            check(L.isr_tuning_set(k, v), "isr_tuning_set")
        return self

    def __exit__(self, *exc):
        L = lib()
        for k, v in self.old.items():
            L.isr_tuning_set(k, v)
        return False


def set_tuning(**knobs) -> None:
    """Set tuning knobs for the rest of the process (tools/ sweeps); see `tuning`."""
    for k, v in knobs.items():
        check(lib().isr_tuning_set(_capi.TUNE[k], int(v)), "isr_tuning_set")


def set_tile_plan(plan: str | None) -> None:
    """'st,sq,tb' (the old ISR_NN_TILE syntax) or None for the defaults."""
    if plan is None:
        set_tuning(nn_tile_st=0, nn_tile_sq=0, nn_tile_tb=0)
    else:
        st, sq, tb = plan.split(",")
        set_tuning(nn_tile_st=round(float(st) * 1000), nn_tile_sq=round(float(sq) * 1000), nn_tile_tb=int(tb))


def workspace(device: torch.device, nbytes: int, tag: str = "default") -> torch.Tensor:
    """A cached, grow-only scratch buffer per (device, stream, tag).
    While the current stream is being captured into a HIP graph nothing is cached: a buffer allocated during
    capture lives in the graph's private pool, and handing it to later eager calls (or to another capture)
    would share that memory with no ordering — a capture gets a fresh buffer per call, which the graph owns.
    Pre-warm (run the call once eagerly) if the capture should reuse the cached buffer instead."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _workspaces.get(key)
    if buf is not None and buf.numel() >= nbytes:
        return buf
    fresh = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    if not torch.cuda.is_current_stream_capturing():
        _workspaces[key] = fresh
    return fresh


def clear_workspaces() -> None:
    """Drop every cached scratch buffer (e.g. after destroying streams: stream handles are reused as keys)."""
    _workspaces.clear()


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).contiguous()


def _f64c(t: torch.Tensor | None) -> torch.Tensor | None:
    return None if t is None else t.to(torch.float64).contiguous()


@dataclass
class NNResult:
    sum_d: torch.Tensor          # (B,) f64
    sum_d2: torch.Tensor         # (B,) f64
    n_in: torch.Tensor           # (B,) i32
    nn_idx: torch.Tensor | None  # (B, Nq) i32
    nn_d: torch.Tensor | None    # (B, Nq) f64
    cov: torch.Tensor | None     # (B, 16) f64


def nn_batched(qry: torch.Tensor, tgt: torch.Tensor, Tq: torch.Tensor | None = None,
               Tt: torch.Tensor | None = None, radius: float = -1.0, want_idx: bool = False,
               want_dist: bool = False, want_cov: bool = False) -> NNResult:
    """isr_nn_batched: qry (Nq,3) f32, tgt (Nt,3) f32, Tq/Tt (B,3,4) or (B,12) f64 or None."""
    dev = require_cuda(qry, tgt, Tq, Tt)
    qry, tgt, Tq, Tt = _f32c(qry), _f32c(tgt), _f64c(Tq), _f64c(Tt)
    if qry.ndim != 2 or qry.shape[1] != 3 or tgt.ndim != 2 or tgt.shape[1] != 3:
        raise ValueError(f"clouds must be (N,3): got {tuple(qry.shape)} and {tuple(tgt.shape)}")
    B = 1
    for T in (Tq, Tt):
        if T is not None:
            if T.numel() % 12:
                raise ValueError("transforms must be (B,3,4)")
            B = max(B, T.numel() // 12)
    for T in (Tq, Tt):
        if T is not None and T.numel() // 12 != B:
            raise ValueError("Tq and Tt must have the same batch size")
    Nq, Nt = qry.shape[0], tgt.shape[0]
    L = lib()
    sum_d = torch.empty(B, dtype=torch.float64, device=dev)
    sum_d2 = torch.empty(B, dtype=torch.float64, device=dev)
    n_in = torch.empty(B, dtype=torch.int32, device=dev)
    nn_idx = torch.empty((B, Nq), dtype=torch.int32, device=dev) if want_idx else None
    nn_d = torch.empty((B, Nq), dtype=torch.float64, device=dev) if want_dist else None
    cov = torch.empty((B, 16), dtype=torch.float64, device=dev) if want_cov else None
    nbytes = L.isr_nn_batched_workspace_bytes(Nq, Nt, B)
    ws = workspace(dev, nbytes, "nn")
    with torch.cuda.device(dev), _timed("nn_batched", float(B) * Nq * Nt):
        rc = L.isr_nn_batched(ptr(qry), Nq, ptr(tgt), Nt, ptr(Tq), ptr(Tt), B, float(radius),
                              ptr(sum_d), ptr(sum_d2), ptr(n_in), ptr(nn_idx), ptr(nn_d), ptr(cov),
                              ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_nn_batched")
    return NNResult(sum_d, sum_d2, n_in, nn_idx, nn_d, cov)


def icp_point_to_point_batch(sources: torch.Tensor, target: torch.Tensor, state: torch.Tensor, threshold: float,
                             max_iter: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6) -> torch.Tensor:
    """isr_icp_point_to_point_batch: B point-to-point ICP loops against one target in one call, in place on `state`.
    sources (Ns,3) f32 — one source, B starts — or (B,Ns,3); target (Nt,3) f32; state (B,20) f64 contiguous, per item
    T 4x4 row-major (start in, result out) | fitness, inlier_rmse, iterations, correspondences.  Returns `state`."""
    dev = require_cuda(sources, target, state)
    if sources.dtype != torch.float32 or target.dtype != torch.float32 or not (sources.is_contiguous() and target.is_contiguous()):
        raise ValueError("icp_point_to_point_batch: sources and target must be contiguous float32")
    if state.dtype != torch.float64 or state.ndim != 2 or state.shape[1] != 20 or not state.is_contiguous():
        raise ValueError(f"icp_point_to_point_batch: state must be contiguous (B,20) float64, got {tuple(state.shape)} {state.dtype}")
    if target.ndim != 2 or target.shape[1] != 3 or sources.ndim not in (2, 3) or sources.shape[-1] != 3:
        raise ValueError(f"icp_point_to_point_batch: sources {tuple(sources.shape)} must be (Ns,3) or (B,Ns,3), target "
                         f"{tuple(target.shape)} (Nt,3)")
    B, Ns, Nt = state.shape[0], sources.shape[-2], target.shape[0]
    if sources.ndim == 3 and sources.shape[0] != B:
        raise ValueError(f"icp_point_to_point_batch: sources {tuple(sources.shape)} and state {tuple(state.shape)} disagree on B")
    stride = 3 * Ns if sources.ndim == 3 else 0
    L = lib()
    ws = workspace(dev, L.isr_icp_point_to_point_batch_workspace_bytes(Ns, Nt, B), "icp")
    with torch.cuda.device(dev), _timed("icp_batch", float(B) * Ns * Nt * (max_iter + 1)):
        rc = L.isr_icp_point_to_point_batch(ptr(sources), stride, Ns, ptr(target), Nt, B, float(threshold), int(max_iter),
                                            float(rel_fitness), float(rel_rmse), ptr(state), ptr(ws), ws.numel(),
                                            current_stream(dev))
    check(rc, "isr_icp_point_to_point_batch")
    return state


ICP_KERNELS = {"l2": _capi.ICP_L2, "huber": _capi.ICP_HUBER, "tukey": _capi.ICP_TUKEY}


def _icp_plane_args(name, sources, target, normals, state, kernel, check_finite, xp):
    """The shape, dtype and value checks both point-to-plane wrappers share -> (B, Ns, Nt, stride, kernel id)."""
    f32, f64 = (torch.float32, torch.float64) if xp is torch else (np.float32, np.float64)
    contiguous = (lambda a: a.is_contiguous()) if xp is torch else (lambda a: a.flags.c_contiguous)
    if any(a.dtype != f32 or not contiguous(a) for a in (sources, target, normals)):
        raise ValueError(f"{name}: sources, target and target_normals must be contiguous float32")
    if state.dtype != f64 or state.ndim != 2 or state.shape[1] != _capi.ICP_PLANE_STATE_DOUBLES or not contiguous(state):
        raise ValueError(f"{name}: state must be contiguous (B,24) float64, got {tuple(state.shape)} {state.dtype}")
    if target.ndim != 2 or target.shape[1] != 3 or sources.ndim not in (2, 3) or sources.shape[-1] != 3:
        raise ValueError(f"{name}: sources {tuple(sources.shape)} must be (Ns,3) or (B,Ns,3), target {tuple(target.shape)} (Nt,3)")
    if tuple(normals.shape) != tuple(target.shape):
        raise ValueError(f"{name}: target_normals {tuple(normals.shape)} must have the target's shape {tuple(target.shape)}")
    B, Ns, Nt = state.shape[0], sources.shape[-2], target.shape[0]
    if sources.ndim == 3 and sources.shape[0] != B:
        raise ValueError(f"{name}: sources {tuple(sources.shape)} and state {tuple(state.shape)} disagree on B")
    if kernel not in ICP_KERNELS:
        raise ValueError(f"{name}: kernel {kernel!r} must be one of {sorted(ICP_KERNELS)}")
    if check_finite:
        for what, a in (("sources", sources), ("target", target), ("target_normals", normals), ("state[:, :12]", state[:, :12])):
            if not bool(xp.isfinite(a).all()):
                raise ValueError(f"{name}: non-finite values in {what} (finite inputs are a precondition)")
    return B, Ns, Nt, (3 * Ns if sources.ndim == 3 else 0), ICP_KERNELS[kernel]


def icp_point_to_plane_batch(sources: torch.Tensor, target: torch.Tensor, target_normals: torch.Tensor, state: torch.Tensor,
                             threshold: float, max_iter: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6,
                             kernel: str = "tukey", k: float = 1.0, check_finite: bool = False) -> torch.Tensor:
    """isr_icp_point_to_plane_batch (include/isr_icp_plane.h states the rule): B point-to-plane ICP loops with robust weights
    against one target in one call, in place on `state`.  sources (Ns,3) f32 — one source, B starts — or (B,Ns,3); target and
    target_normals (Nt,3) f32; state (B,24) f64 contiguous, per item T 4x4 row-major (start in, result out) | fitness,
    inlier_rmse, iterations, correspondences | status, sum w r^2, 0, 0.  kernel: "l2", "huber" or "tukey" with scale k.
    Nothing synchronises but check_finite, which refuses non-finite inputs.  Returns `state`."""
    dev = require_cuda(sources, target, target_normals, state)
    B, Ns, Nt, stride, kid = _icp_plane_args("icp_point_to_plane_batch", sources, target, target_normals, state, kernel,
                                             check_finite, torch)
    if B == 0:                  # nothing to do (an empty tensor has no address to hand over)
        return state
    L = lib()
    ws = workspace(dev, L.isr_icp_point_to_plane_batch_workspace_bytes(Ns, Nt, B), "icp")
    with torch.cuda.device(dev), _timed("icp_plane_batch", float(B) * Ns * Nt * (max_iter + 1)):
        rc = L.isr_icp_point_to_plane_batch(ptr(sources), stride, Ns, ptr(target), ptr(target_normals), Nt, B, float(threshold),
                                            int(max_iter), float(rel_fitness), float(rel_rmse), kid, float(k), ptr(state),
                                            ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_icp_point_to_plane_batch")
    return state


def icp_point_to_plane_batch_host(sources, target, target_normals, state, threshold: float, max_iter: int = 30,
                                  rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, kernel: str = "tukey", k: float = 1.0,
                                  check_finite: bool = False):
    """isr_icp_point_to_plane_batch_host: the same loop as host code with an f64 brute-force search, NumPy arrays of the
    shapes icp_point_to_plane_batch takes, in place on `state`: the same bits.  For tests and CPU users."""
    for a in (sources, target, target_normals, state):
        if not isinstance(a, np.ndarray):
            raise ValueError("icp_point_to_plane_batch_host: NumPy arrays only (device tensors go to icp_point_to_plane_batch)")
    B, Ns, Nt, stride, kid = _icp_plane_args("icp_point_to_plane_batch_host", sources, target, target_normals, state, kernel,
                                             check_finite, np)
    if B == 0:
        return state
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_icp_point_to_plane_batch_host(hp(sources), stride, Ns, hp(target), hp(target_normals), Nt, B, float(threshold),
                                                  int(max_iter), float(rel_fitness), float(rel_rmse), kid, float(k), hp(state)),
          "isr_icp_point_to_plane_batch_host")
    return state


def _seq_refit_args(name, p3d, p2d, counts, frame_w, K, G, state, kernel, xp):
    """The shape and dtype checks both sequence-refit wrappers share -> (n, cap, kernel id)."""
    f32, f64, i32 = (torch.float32, torch.float64, torch.int32) if xp is torch else (np.float32, np.float64, np.int32)
    contiguous = (lambda a: a.is_contiguous()) if xp is torch else (lambda a: a.flags.c_contiguous)
    if p3d.ndim != 3 or p3d.shape[2] != 3 or p2d.ndim != 3 or tuple(p2d.shape) != (p3d.shape[0], p3d.shape[1], 2):
        raise ValueError(f"{name}: p3d {tuple(p3d.shape)} must be (n, cap, 3) and p2d {tuple(p2d.shape)} (n, cap, 2)")
    n, cap = p3d.shape[0], p3d.shape[1]
    if p3d.dtype != f32 or p2d.dtype != f32 or not contiguous(p3d) or not contiguous(p2d):
        raise ValueError(f"{name}: p3d and p2d must be contiguous float32")
    if counts.dtype != i32 or tuple(counts.shape) != (n,) or not contiguous(counts):
        raise ValueError(f"{name}: counts must be contiguous (n,) int32, got {tuple(counts.shape)} {counts.dtype}")
    for what, a, shape in (("K", K, (n, 9)), ("G", G, (n, 12)), ("state", state, (_capi.SEQ_REFIT_STATE_DOUBLES,)),
                           ("frame_w", frame_w, (n,))):
        if a is None and what == "frame_w":
            continue
        if a.dtype != f64 or tuple(a.shape) != shape or not contiguous(a):
            raise ValueError(f"{name}: {what} must be contiguous {shape} float64, got {tuple(a.shape)} {a.dtype}")
    if cap < 1:
        raise ValueError(f"{name}: cap must be at least 1")
    if kernel not in ICP_KERNELS:
        raise ValueError(f"{name}: kernel {kernel!r} must be one of {sorted(ICP_KERNELS)}")
    return n, cap, ICP_KERNELS[kernel]


def seq_refit(p3d: torch.Tensor, p2d: torch.Tensor, counts: torch.Tensor, K: torch.Tensor, G: torch.Tensor, state: torch.Tensor,
              frame_w: torch.Tensor | None = None, kernel: str = "tukey", k: float = 6.0, max_iter: int = 30,
              tol_r: float = 1e-10, tol_t: float = 1e-8, workspace_buf: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """isr_seq_refit (include/isr_seq_refit.h states the rule): one robust Gauss-Newton for the sequence transform Y over the
    reprojection residuals of every frame's matches, in place on `state`.  p3d (n, cap, 3) f32, p2d (n, cap, 2) f32, counts
    (n,) i32, K (n, 9) f64, G (n, 12) f64 [R_i | t_i], state (24,) f64 = Y 4x4 (start in, result out) | mean a, rms, passes,
    rows | status, sum w r.r, 0, 0; frame_w (n,) f64 or None; workspace_buf: a caller's uint8 scratch instead of the cached one
    (whatever it holds).  Nothing synchronises.  Returns (state, frame_stats (n, 4))."""
    dev = require_cuda(p3d, p2d, counts, K, G, state, *(() if frame_w is None else (frame_w,)))
    n, cap, kid = _seq_refit_args("seq_refit", p3d, p2d, counts, frame_w, K, G, state, kernel, torch)
    stats = torch.empty((n, _capi.SEQ_REFIT_FRAME_STATS), dtype=torch.float64, device=dev)
    L = lib()
    nbytes = L.isr_seq_refit_workspace_bytes(n, cap)
    ws = None if not n else workspace_buf if workspace_buf is not None else workspace(dev, nbytes, "seq_refit")
    with torch.cuda.device(dev), _timed("seq_refit", float(n) * cap * (max_iter + 1)):
        rc = L.isr_seq_refit(ptr(p3d), ptr(p2d), ptr(counts), ptr(frame_w), ptr(K), ptr(G), n, cap, kid, float(k), int(max_iter),
                             float(tol_r), float(tol_t), ptr(state), ptr(stats), ptr(ws), ws.numel() if n else 0,
                             current_stream(dev))
    check(rc, "isr_seq_refit")
    return state, stats


def seq_refit_host(p3d, p2d, counts, K, G, state, frame_w=None, kernel: str = "tukey", k: float = 6.0, max_iter: int = 30,
                   tol_r: float = 1e-10, tol_t: float = 1e-8):
    """isr_seq_refit_host: the same loop as host code, NumPy arrays of the shapes seq_refit takes, in place on `state`: the
    same bits.  For tests and CPU users.  Returns (state, frame_stats (n, 4))."""
    for a in (p3d, p2d, counts, K, G, state, *(() if frame_w is None else (frame_w,))):
        if not isinstance(a, np.ndarray):
            raise ValueError("seq_refit_host: NumPy arrays only (device tensors go to seq_refit)")
    n, cap, kid = _seq_refit_args("seq_refit_host", p3d, p2d, counts, frame_w, K, G, state, kernel, np)
    stats = np.empty((n, _capi.SEQ_REFIT_FRAME_STATS), np.float64)
    hp = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_seq_refit_host(hp(p3d), hp(p2d), hp(counts), hp(frame_w), hp(K), hp(G), n, cap, kid, float(k), int(max_iter),
                                   float(tol_r), float(tol_t), hp(state), hp(stats)), "isr_seq_refit_host")
    return state, stats


def seq_refit_sums_host(p3d, p2d, counts, K, G, Y, frame_w=None, kernel: str = "tukey", k: float = 6.0):
    """isr_seq_refit_sums_host: the 31 sums of one pass at Y (4x4 f64), formed as the loop forms them, NumPy arrays.
    Returns (sums (31,), frame_stats (n, 4)).  For tests."""
    state = np.zeros(_capi.SEQ_REFIT_STATE_DOUBLES)
    state[:16] = np.asarray(Y, np.float64).reshape(16)
    n, cap, kid = _seq_refit_args("seq_refit_sums_host", p3d, p2d, counts, frame_w, K, G, state, kernel, np)
    sums, stats = np.empty(31), np.empty((n, _capi.SEQ_REFIT_FRAME_STATS), np.float64)
    hp = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_seq_refit_sums_host(hp(p3d), hp(p2d), hp(counts), hp(frame_w), hp(K), hp(G), n, cap, kid, float(k), hp(state),
                                        hp(sums), hp(stats)), "isr_seq_refit_sums_host")
    return sums, stats


@dataclass
class DistField:
    """Distances from the cell centres of a uniform grid to a (static) cloud: what isr_adds_bounds reads."""
    field: torch.Tensor       # (nz, ny, nx) f32 device
    grid_min: np.ndarray      # (3,) f64 host: the corner of cell (0, 0, 0)
    h: float                  # cell edge
    dims: tuple               # (nx, ny, nz)
    bbox: np.ndarray          # (6,) f32 host: the cloud's bounding box, lo xyz then hi xyz
    n_points: int


def dist_field(cloud: torch.Tensor, cells: int = 128, margin: float | None = None) -> DistField:
    """Exact distances from the centres of a cells^3-ish grid around `cloud` (N,3) to the cloud, through isr_nn_batched.
    margin: how far beyond the cloud's bounding box the grid reaches (default: a quarter of its longest extent)."""
    dev = require_cuda(cloud)
    c = _f32c(cloud)
    lo, hi = c.min(dim=0).values.double().cpu().numpy(), c.max(dim=0).values.double().cpu().numpy()
    ext = hi - lo
    m = float(0.25 * ext.max()) if margin is None else float(margin)
    h = float((ext.max() + 2.0 * m) / cells)
    gmin = lo - m
    dims = tuple(int(np.ceil((ext[a] + 2.0 * m) / h)) for a in range(3))
    ax = [gmin[a] + h * (torch.arange(dims[a], device=dev, dtype=torch.float64) + 0.5) for a in range(3)]
    zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    centres = torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3).to(torch.float32).contiguous()
    # the centres as f32 are what the field is exact for: their rounding (<= 4e-6 mm at object scale) sits inside the slack
    # every user of the bounds keeps around the threshold
    parts = [nn_batched(centres[s0:s0 + (1 << 20)], c, want_dist=True).nn_d[0] for s0 in range(0, centres.shape[0], 1 << 20)]
    field = torch.cat(parts).to(torch.float32).reshape(dims[2], dims[1], dims[0]).contiguous()
    return DistField(field, np.asarray(gmin, np.float64), h, dims, np.concatenate([lo, hi]).astype(np.float32), int(c.shape[0]))


def adds_bounds(verts: torch.Tensor, Tq: torch.Tensor, Tt: torch.Tensor | None, fld: DistField):
    """isr_adds_bounds: per batch item b bounds of sum_v dist(Tt[b]^-1 Tq[b] v, cloud) — isr_nn_batched's sum_d for queries
    `verts` against the field's cloud — as (lb_sum, ub_sum) f64 device tensors: wider, still finite, for vertices off the grid;
    (0, +inf) — a bracket that decides nothing — for an item whose Tt is not rigid to within eta = 3 max|R^T R - I| <= 0.009."""
    import ctypes
    dev = require_cuda(verts, Tq, Tt, fld.field)
    v, Tq, Tt = _f32c(verts), _f64c(Tq), _f64c(Tt)
    if v.ndim != 2 or v.shape[1] != 3 or Tq.numel() % 12 or (Tt is not None and Tt.numel() != Tq.numel()):
        raise ValueError(f"adds_bounds: verts {tuple(v.shape)}, Tq {tuple(Tq.shape)}, Tt {None if Tt is None else tuple(Tt.shape)}")
    B = Tq.numel() // 12
    lb = torch.empty(B, dtype=torch.float64, device=dev)
    ub = torch.empty(B, dtype=torch.float64, device=dev)
    if B == 0:
        return lb, ub
    gmin = (ctypes.c_double * 3)(*[float(x) for x in fld.grid_min])
    bbox = (ctypes.c_float * 6)(*[float(x) for x in fld.bbox])
    with torch.cuda.device(dev), _timed("adds_bounds", float(B) * v.shape[0]):
        rc = lib().isr_adds_bounds(ptr(v), v.shape[0], ptr(Tq), ptr(Tt), B, ptr(fld.field), ctypes.cast(gmin, ctypes.c_void_p),
                                   float(fld.h), fld.dims[0], fld.dims[1], fld.dims[2], ctypes.cast(bbox, ctypes.c_void_p),
                                   ptr(lb), ptr(ub), current_stream(dev))
    check(rc, "isr_adds_bounds")
    return lb, ub


def rel_pose_table(R: torch.Tensor, t: torch.Tensor, mode: int, i0: int = 0,
                   i1: int | None = None) -> torch.Tensor:
    """isr_rel_pose_table: rows [i0,i1) of the n x n relative-pose table as (rows, n, 3, 4) f64."""
    dev = require_cuda(R, t)
    R, t = _f64c(R).reshape(-1, 9), _f64c(t).reshape(-1, 3)
    n = R.shape[0]
    i1 = n if i1 is None else i1
    out = torch.empty((i1 - i0, n, 3, 4), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib().isr_rel_pose_table(ptr(R), ptr(t), n, i0, i1, mode, ptr(out), current_stream(dev))
    check(rc, "isr_rel_pose_table")
    return out


def _pad_cols(t: torch.Tensor, D: int) -> torch.Tensor:
    if t.shape[1] == D:
        return t.contiguous()
    out = torch.zeros((t.shape[0], D), dtype=t.dtype, device=t.device)
    out[:, : t.shape[1]] = t
    return out


LOG2E = 1.4426950408889634


def prescale_queries_log2(queries: torch.Tensor) -> torch.Tensor:
    """f32 descriptors -> bf16(queries * log2 e): the input of corr_argmax(..., log2_prescaled=True).
    One rounding, as for a plain .bfloat16(); a conversion, not part of the measured path."""
    return (queries.to(torch.float32) * LOG2E).to(torch.bfloat16)


@dataclass
class CorrCall:
    """An isr_corr_argmax call whose opening half has been enqueued (corr_argmax_open): what corr_argmax_close needs."""
    q: torch.Tensor
    k: torch.Tensor
    P: int
    N: int
    Dp: int
    dtype: int
    idx: torch.Tensor
    logp: torch.Tensor
    lse: torch.Tensor | None
    rows_per_image: int
    n_rows: torch.Tensor | None
    hist: torch.Tensor | None
    ws: torch.Tensor
    dev: torch.device

    def outputs(self):
        out = (self.idx, self.logp) if self.lse is None else (self.idx, self.logp, self.lse)
        return out if self.hist is None else out + (self.hist,)


def _corr_prepare(queries, keys, want_lse, log2_prescaled, screened, rows_per_image, n_rows, ws_tag) -> CorrCall:
    dev = require_cuda(queries, keys, n_rows)
    if queries.ndim != 2 or keys.ndim != 2 or queries.shape[1] != keys.shape[1]:
        raise ValueError(f"queries {tuple(queries.shape)} / keys {tuple(keys.shape)} must be (P,D),(N,D)")
    P, D = queries.shape
    N = keys.shape[0]
    if P == 0 or N == 0:
        raise ValueError("empty queries or keys")
    if screened and not log2_prescaled:
        raise ValueError("screened needs log2-prescaled bf16 queries")
    if queries.dtype == torch.bfloat16 and keys.dtype == torch.bfloat16:
        dtype = (_capi.DTYPE_BF16_LOG2_SCREENED if screened else _capi.DTYPE_BF16_LOG2) if log2_prescaled else _capi.DTYPE_BF16
        Dp = next((d for d in (16, 32, 64, 128) if d >= D), None)
        if Dp is None:
            raise ValueError(f"bf16 path supports D <= 128, got {D}")
    else:
        if log2_prescaled:
            raise ValueError("log2_prescaled needs bf16 queries and keys")
        dtype = _capi.DTYPE_F32
        queries, keys = queries.to(torch.float32), keys.to(torch.float32)
        Dp = D
        if D > 128:
            raise ValueError(f"f32 path supports D <= 128, got {D}")
    q, k = _pad_cols(queries, Dp), _pad_cols(keys, Dp)
    idx = torch.empty(P, dtype=torch.int32, device=dev)
    logp = torch.empty(P, dtype=torch.float32, device=dev)
    lse = torch.empty(P, dtype=torch.float32, device=dev) if want_lse else None
    ws = workspace(dev, lib().isr_corr_argmax_workspace_bytes(P, N, Dp, dtype), ws_tag)
    hist = None
    if rows_per_image is not None:
        if rows_per_image <= 0 or P % rows_per_image:
            raise ValueError(f"corr_argmax: P={P} is not a whole number of images of {rows_per_image} rows")
        if n_rows is not None and (n_rows.dtype != torch.int32 or n_rows.numel() != P // rows_per_image):
            raise ValueError("corr_argmax: n_rows must be (images,) int32")
        hist = torch.empty((P // rows_per_image, 2048), dtype=torch.int32, device=dev)
    return CorrCall(q, k, P, N, Dp, dtype, idx, logp, lse, int(rows_per_image or 1), n_rows, hist, ws, dev)


def _corr_launch(c: CorrCall, phase: int, what: str, work: float) -> None:
    L = lib()
    with torch.cuda.device(c.dev), _timed(what, work):
        if phase == 3 and c.hist is None:
            rc = L.isr_corr_argmax(ptr(c.q), ptr(c.k), c.P, c.N, c.Dp, c.Dp, c.Dp, c.dtype, ptr(c.idx), ptr(c.logp), ptr(c.lse),
                                   ptr(c.ws), c.ws.numel(), current_stream(c.dev))
        elif phase == 3:
            rc = L.isr_corr_argmax_digits(ptr(c.q), ptr(c.k), c.P, c.N, c.Dp, c.Dp, c.Dp, c.dtype, ptr(c.idx), ptr(c.logp), ptr(c.lse),
                                          c.rows_per_image, ptr(c.n_rows), ptr(c.hist), ptr(c.ws), c.ws.numel(), current_stream(c.dev))
        else:
            rc = L.isr_corr_argmax_phase(ptr(c.q), ptr(c.k), c.P, c.N, c.Dp, c.Dp, c.Dp, c.dtype, ptr(c.idx), ptr(c.logp), ptr(c.lse),
                                         c.rows_per_image, ptr(c.n_rows), ptr(c.hist), phase, ptr(c.ws), c.ws.numel(),
                                         current_stream(c.dev))
    check(rc, "isr_corr_argmax")
    global _last_corr
    _last_corr = (c.ws, c.P, c.N, c.dtype, c.dev)


def corr_argmax(queries: torch.Tensor, keys: torch.Tensor, want_lse: bool = False,
                log2_prescaled: bool = False, screened: bool = False, rows_per_image: int | None = None,
                n_rows: torch.Tensor | None = None):
    """isr_corr_argmax.  queries (P,D), keys (N,D); bf16 tensors take the bf16 MFMA path, f32
    tensors the exact f32 MFMA path (f16/f64 are converted to f32).  Zero columns are appended
    where the kernel needs a padded D (exact: they add 0 to every logit).
    log2_prescaled: the bf16 queries already carry a factor log2(e) (prescale_queries_log2): the
    kernel works in log2 units with the -M2 reference folded into the MFMA contraction; outputs are
    still natural-log.
    screened (with log2_prescaled): ISR_DTYPE_BF16_LOG2_SCREENED — the rows also go through a block-scaled FP6 screen, and
    pieces of the log-sum-exp proven to lie more than T = 21 + ceil(log2 N) log2 units below the query's maximum are never
    formed (indices stay exact, lse moves by < 5e-7; D = 64 only, other shapes run unscreened).  For peaked softmaxes.
    rows_per_image: isr_corr_argmax_digits — the rows are P / rows_per_image images whose top-80 % cut follows; the call also
    returns digit_hist (images, 2048) i32, the first histogram of that cut's radix select over logp (of image b's first
    n_rows[b] rows; n_rows None: all), formed where logp is written: pass it to select_top_batch(..., digit_hist=...).
    Returns idx (P,) i32, logp (P,) f32[, lse (P,) f32][, digit_hist] on the device."""
    c = _corr_prepare(queries, keys, want_lse, log2_prescaled, screened, rows_per_image, n_rows, "corr")
    _corr_launch(c, 3, "corr_argmax", 2.0 * c.P * c.N * c.Dp)
    return c.outputs()


def corr_argmax_open(queries: torch.Tensor, keys: torch.Tensor, want_lse: bool = False, log2_prescaled: bool = False,
                     screened: bool = False, rows_per_image: int | None = None, n_rows: torch.Tensor | None = None,
                     ws_tag: str = "corr") -> CorrCall:
    """isr_corr_argmax_phase, phase 1: pre-processing, key norms and the chip-filling kernel(s) of a corr_argmax call, enqueued
    on the current stream.  corr_argmax_close(call) enqueues the closing kernels (fallback, finalize, recheck, merge) — on
    whatever stream is current then, ordered behind this one by the caller (an event) — and returns corr_argmax's outputs.
    The workspace (cached per stream and ws_tag) must not be opened again before its close has finished: alternate two tags."""
    c = _corr_prepare(queries, keys, want_lse, log2_prescaled, screened, rows_per_image, n_rows, ws_tag)
    _corr_launch(c, 1, "corr_argmax", 2.0 * c.P * c.N * c.Dp)
    return c


def corr_argmax_close(call: CorrCall):
    """isr_corr_argmax_phase, phase 2, for a call opened by corr_argmax_open: the outputs are complete when it has run."""
    _corr_launch(call, 2, "corr_close", 0.0)
    return call.outputs()


def corr_lse(queries: torch.Tensor, keys: torch.Tensor, log2_prescaled: bool = False, screened: bool = False) -> torch.Tensor:
    """The row log-sum-exps of queries @ keys.T alone — pose_refine.py:56's denominator image, estimate_pose's row sums
    (poseEstSurf.py:68-71) — as an lse-only call of isr_corr_argmax (idx = logp = NULL): no maxima are tracked, no index is
    certified, and the values are the bits corr_argmax(..., want_lse=True) returns."""
    dev = require_cuda(queries, keys)
    if queries.ndim != 2 or keys.ndim != 2 or queries.shape[1] != keys.shape[1]:
        raise ValueError(f"queries {tuple(queries.shape)} / keys {tuple(keys.shape)} must be (P,D),(N,D)")
    P, D = queries.shape
    N = keys.shape[0]
    if P == 0 or N == 0:
        raise ValueError("empty queries or keys")
    if queries.dtype == torch.bfloat16 and keys.dtype == torch.bfloat16:
        dtype = (_capi.DTYPE_BF16_LOG2_SCREENED if screened else _capi.DTYPE_BF16_LOG2) if log2_prescaled else _capi.DTYPE_BF16
        Dp = next((d for d in (16, 32, 64, 128) if d >= D), None)
        if Dp is None:
            raise ValueError(f"bf16 path supports D <= 128, got {D}")
    else:
        if log2_prescaled:
            raise ValueError("log2_prescaled needs bf16 queries and keys")
        dtype = _capi.DTYPE_F32
        queries, keys = queries.to(torch.float32), keys.to(torch.float32)
        Dp = D
        if D > 128:
            raise ValueError(f"f32 path supports D <= 128, got {D}")
    q, k = _pad_cols(queries, Dp), _pad_cols(keys, Dp)
    lse = torch.empty(P, dtype=torch.float32, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_corr_argmax_workspace_bytes(P, N, Dp, dtype), "corr")
    with torch.cuda.device(dev), _timed("corr_lse", 2.0 * P * N * Dp):
        rc = L.isr_corr_argmax(ptr(q), ptr(k), P, N, Dp, Dp, Dp, dtype, None, None, ptr(lse), ptr(ws), ws.numel(),
                               current_stream(dev))
    check(rc, "isr_corr_argmax (lse only)")
    return lse


def corr_topk(queries: torch.Tensor, keys: torch.Tensor, k: int):
    """getCors with leaves = k > 1 (inference.py:145-149): per query the k largest entries of log_softmax(queries @ keys.T)
    and their keys — isr_corr_topk behind an lse-only K1 call; the (P, N) matrix is never formed.  Any float dtype (bf16 /
    f16 rows are widened exactly); 1 <= k <= 8.  Returns idx (P, k) int32, vals (P, k) f32 on the device, descending,
    equal values by ascending key."""
    dev = require_cuda(queries, keys)
    if queries.ndim != 2 or keys.ndim != 2 or queries.shape[1] != keys.shape[1]:
        raise ValueError(f"queries {tuple(queries.shape)} / keys {tuple(keys.shape)} must be (P,D),(N,D)")
    if not 1 <= int(k) <= 8:
        raise ValueError(f"leaves = {k}: 1 .. 8 are supported without materialising the matrix")
    q, kk = _f32c(queries), _f32c(keys)
    P, D = q.shape
    N = kk.shape[0]
    if P == 0 or N == 0:
        raise ValueError("empty queries or keys")
    if D > 128:
        raise ValueError(f"D <= 128, got {D}")
    lse = corr_lse(q, kk)
    idx = torch.empty((P, int(k)), dtype=torch.int32, device=dev)
    vals = torch.empty((P, int(k)), dtype=torch.float32, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_corr_topk_workspace_bytes(P, N), "corr_topk")
    with torch.cuda.device(dev):
        rc = L.isr_corr_topk(ptr(q), ptr(kk), P, N, D, D, D, int(k), ptr(lse), ptr(idx), ptr(vals), ptr(ws), ws.numel(),
                             current_stream(dev))
    check(rc, "isr_corr_topk")
    return idx, vals


_last_corr = None


def corr_clock_mhz() -> float:
    """Diagnostics: the shader clock (MHz) the last bf16 corr_argmax launch held (0.0 for the f32 path)."""
    import ctypes
    if _last_corr is None:
        return 0.0
    ws, P, N, dtype, dev = _last_corr
    out = ctypes.c_double(0.0)
    with torch.cuda.device(dev):
        rc = lib().isr_corr_argmax_clock_mhz(ptr(ws), ws.numel(), P, N, dtype, ctypes.addressof(out), current_stream(dev))
    check(rc, "isr_corr_argmax_clock_mhz")
    return float(out.value)


def corr_recheck_count() -> int:
    """Diagnostics: how many queries of the last corr_argmax call were decided by the exact recheck
    (-1 on the f32 path).  Synchronises the current stream."""
    import ctypes
    if _last_corr is None:
        return -1
    ws, P, N, dtype, dev = _last_corr
    out = ctypes.c_int32(-1)
    with torch.cuda.device(dev):
        rc = lib().isr_corr_argmax_recheck_count(ptr(ws), ws.numel(), P, N, dtype, ctypes.addressof(out),
                                                 current_stream(dev))
    check(rc, "isr_corr_argmax_recheck_count")
    return int(out.value)


def corr_quantize_fp6(rows: torch.Tensor):
    """isr_corr_quantize_fp6 (parity hook of the screened K1 route): rows (R, 64) bf16 on the device ->
    (image (R, 64) uint8, norms (R, 2) f32 {|x|, |x - x~|}, maxima (2,) f32 {max |x - x~|^2, max |x~|^2})."""
    dev = require_cuda(rows)
    if rows.ndim != 2 or rows.shape[1] != 64 or rows.dtype != torch.bfloat16:
        raise ValueError(f"rows must be (R, 64) bf16, got {tuple(rows.shape)} {rows.dtype}")
    rows = rows.contiguous()
    R = rows.shape[0]
    out = torch.empty((R, 64), dtype=torch.uint8, device=dev)
    nrm = torch.empty((R, 2), dtype=torch.float32, device=dev)
    kmax = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().isr_corr_quantize_fp6(ptr(rows), R, 64, ptr(out), ptr(nrm), ptr(kmax), current_stream(dev))
    check(rc, "isr_corr_quantize_fp6")
    return out, nrm, kmax


def corr_screen_redone() -> tuple[int, int]:
    """Diagnostics of the last screened corr_argmax call: (tile items — 32 queries x 32 keys — fetched again and redone on the
    bf16 matrix cores behind the FP6 screen, 256-query blocks handed to the dense kernel); zeros on the unscreened routes.
    Synchronises the current stream."""
    import ctypes
    if _last_corr is None:
        return 0, 0
    ws, P, N, dtype, dev = _last_corr
    out = (ctypes.c_longlong * 2)(0, 0)
    with torch.cuda.device(dev):
        rc = lib().isr_corr_argmax_screen_redone(ptr(ws), ws.numel(), P, N, dtype, ctypes.addressof(out), current_stream(dev))
    check(rc, "isr_corr_argmax_screen_redone")
    return int(out[0]), int(out[1])


def corr_recheck_count_f32(D: int) -> int:
    """Diagnostics: the length of the f32-chain recheck list of the last f32 corr_argmax call with D columns, under the
    knob setting still in force (-1 when that call took the f32-MFMA chain kernel).  Synchronises the current stream."""
    import ctypes
    if _last_corr is None:
        return -1
    ws, P, N, dtype, dev = _last_corr
    if dtype != _capi.DTYPE_F32:
        return -1
    out = ctypes.c_int32(-1)
    with torch.cuda.device(dev):
        rc = lib().isr_corr_argmax_recheck_count_f32(ptr(ws), ws.numel(), P, N, int(D), ctypes.addressof(out),
                                                     current_stream(dev))
    check(rc, "isr_corr_argmax_recheck_count_f32")
    return int(out.value)


def select_top(logp: torch.Tensor, frac: float = 0.8, min_n: int = 500, n_dev: torch.Tensor | None = None):
    """select_top_batch of one image: logp (P,) -> keep (P,) i32 (first M entries valid, ascending), M_dev (1,) i32,
    thr (1,) f32.  n_dev: (1,) i32 on the device — only the first n_dev values are the input."""
    keep, M_dev, thr = select_top_batch(logp.reshape(1, -1), frac, min_n, n_dev)
    return keep[0], M_dev, thr


def prep_queries(feat: torch.Tensor, mask: torch.Tensor, c0: int = 0, D: int | None = None, step: int = 3,
                 dtype: str = "bf16_log2"):
    """prep_queries_batch of one crop: feat (H, W, C) or (1, H, W, C) f32; mask (H, W) or (H, W, k) uint8.
    Returns Q (S, Dpad), pix_xy (S, 2) f32, n_dev (1,) i32."""
    Q, pix, n_dev = prep_queries_batch(feat.reshape(1, *feat.shape[-3:]), mask[None], c0, D, step, dtype)
    return Q[0], pix[0], n_dev


def prep_queries_batch(feat: torch.Tensor, mask: torch.Tensor, c0: int = 0, D: int | None = None, step: int = 3,
                       dtype: str = "bf16_log2"):
    """isr_prep_queries_batch: the network's channels-last feature maps -> K1's query operand, a GROUP of crops in three
    launches.  feat (B, H, W, C) f32; mask (B, H, W) or (B, H, W, k) uint8 (channel 0 is used, as cropMask[:, :, 0]);
    dtype 'bf16' | 'bf16_log2' | 'f32'.  Returns Q (B, S, Dpad) with zero rows past each image's count, pix_xy (B, S, 2)
    f32, n_dev (B,) i32 — S = capacity = ceil(H/step) * ceil(W/step)."""
    dev = require_cuda(feat, mask)
    if feat.ndim != 4:
        raise ValueError(f"prep_queries_batch: feat {tuple(feat.shape)} must be (B, H, W, C)")
    feat = _f32c(feat)
    B, H, W, C = feat.shape
    D = C - c0 if D is None else D
    if mask.dtype != torch.uint8:
        mask = (mask != 0).to(torch.uint8)
    mask = mask.contiguous()
    stride = 1 if mask.ndim == 3 else mask.shape[3]
    if tuple(mask.shape[:3]) != (B, H, W):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the feature maps {(B, H, W)}")
    code = {"bf16": _capi.DTYPE_BF16, "bf16_log2": _capi.DTYPE_BF16_LOG2, "f32": _capi.DTYPE_F32}[dtype]
    Dpad = D if dtype == "f32" else (16 if D <= 16 else 32 if D <= 32 else 64 if D <= 64 else 128)
    if D > 128 or (dtype == "f32" and D > 64):
        raise ValueError(f"D={D} not supported by K1")
    S = ((H + step - 1) // step) * ((W + step - 1) // step)
    Q = torch.empty((B, S, Dpad), dtype=torch.float32 if dtype == "f32" else torch.bfloat16, device=dev)
    pix = torch.zeros((B, S, 2), dtype=torch.float32, device=dev)
    n_dev = torch.empty(B, dtype=torch.int32, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_prep_queries_batch_workspace_bytes(H, W, step, B), "prep")
    with torch.cuda.device(dev):
        rc = L.isr_prep_queries_batch(ptr(feat), B, H, W, C, int(c0), int(D), ptr(mask), int(stride), int(step), code, Dpad,
                                      ptr(Q), ptr(pix), ptr(n_dev), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_prep_queries_batch")
    return Q, pix, n_dev


IMAGENET_MEAN = (0.485, 0.456, 0.406)      # normalize(), inference.py:135-141
IMAGENET_STD = (0.229, 0.224, 0.225)


def mask_bbox(mask: torch.Tensor) -> torch.Tensor:
    """isr_mask_bbox: mask (B, H, W[, C]) u8 on the device -> (B, 4) i32 {x, y, w, h} (cv2.boundingRect of channel 0)."""
    dev = require_cuda(mask)
    m = mask if mask.ndim == 4 else mask[..., None]
    m = m.contiguous()
    B, H, W, C = m.shape
    out = torch.empty((B, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().isr_mask_bbox(ptr(m), B, H, W, C, ptr(out), current_stream(dev))
    check(rc, "isr_mask_bbox")
    return out


def crop_normalize(rgb: torch.Tensor, mask: torch.Tensor, M, out_size: int = 224, use_mask: bool = True,
                   mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """isr_crop_normalize: rgb (B, H, W, 3) u8, mask (B, H, W[, C]) u8 on the device, M (B, 2, 3) host f64 (the
    reference's source -> crop affine) -> inputIM (B, 3, r, r) f32, cropMask (B, r, r) u8."""
    import ctypes
    import numpy as np
    dev = require_cuda(rgb, mask)
    rgb = rgb.contiguous()
    m = (mask if mask.ndim == 4 else mask[..., None]).contiguous()
    B, H, W, _ = rgb.shape
    if rgb.dtype != torch.uint8 or m.dtype != torch.uint8 or tuple(m.shape[:3]) != (B, H, W) or rgb.shape[3] != 3:
        raise ValueError(f"crop_normalize: rgb {tuple(rgb.shape)} {rgb.dtype} / mask {tuple(m.shape)} {m.dtype}")
    Mh = np.ascontiguousarray(np.asarray(M, np.float64).reshape(B, 6))
    mu = (ctypes.c_double * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_double * 3)(*[float(v) for v in std])
    out = torch.empty((B, 3, out_size, out_size), dtype=torch.float32, device=dev)
    cm = torch.empty((B, out_size, out_size), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib().isr_crop_normalize(ptr(rgb), ptr(m), B, H, W, m.shape[3], Mh.ctypes.data_as(ctypes.c_void_p), int(out_size),
                                      int(bool(use_mask)), ctypes.cast(mu, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p),
                                      ptr(out), ptr(cm), current_stream(dev))
    check(rc, "isr_crop_normalize")
    return out, cm


def gather_corr(idx, keep, M_dev, pts, pix_xy):
    """gather_corr_batch of one image: idx, keep (P,), pix_xy (P, 2) -> p3d (P,3) f32, p2d (P,2) f32 (first M rows valid)."""
    p3d, p2d = gather_corr_batch(idx.reshape(1, -1), keep.reshape(1, -1), M_dev, pts, pix_xy)
    return p3d[0], p2d[0]


def _kcam(K) -> "ctypes.Array":
    import ctypes
    import numpy as np
    k = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(9))
    return (ctypes.c_double * 9)(*k.tolist())


def _m_dev(M, dev, cap):
    if isinstance(M, torch.Tensor):
        return M
    return torch.tensor([cap if M is None else int(M)], dtype=torch.int32, device=dev)


def p3p_hypotheses(p3d, p2d, Kcam, H: int, seed: int, M_dev=None, want_samples: bool = False):
    import ctypes
    dev = require_cuda(p3d, p2d)
    p3d, p2d = _f32c(p3d), _f32c(p2d)
    cap = p3d.shape[0]
    M_dev = _m_dev(M_dev, dev, cap)
    Rt = torch.empty((H, 3, 4), dtype=torch.float64, device=dev)
    ok = torch.empty(H, dtype=torch.uint8, device=dev)
    smp = torch.empty((H, 4), dtype=torch.int32, device=dev) if want_samples else None
    k = _kcam(Kcam)
    with torch.cuda.device(dev):
        rc = lib().isr_p3p_hypotheses(ptr(p3d), ptr(p2d), ptr(M_dev), cap, ctypes.cast(k, ctypes.c_void_p),
                                      H, seed & 0xFFFFFFFFFFFFFFFF, ptr(Rt), ptr(ok), ptr(smp),
                                      current_stream(dev))
    check(rc, "isr_p3p_hypotheses")
    return (Rt, ok, smp) if want_samples else (Rt, ok)


def p3p_all_roots(X, uv, Kcam):
    """isr_p3p_all_roots (diagnostics): X (S,3,3), uv (S,3,2) f64 on the device -> poses (S,4,3,4), n (S,)."""
    import ctypes
    dev = require_cuda(X, uv)
    X, uv = _f64c(X), _f64c(uv)
    S = X.shape[0]
    poses = torch.zeros((S, 4, 3, 4), dtype=torch.float64, device=dev)
    n = torch.zeros(S, dtype=torch.int32, device=dev)
    k = _kcam(Kcam)
    with torch.cuda.device(dev):
        rc = lib().isr_p3p_all_roots(ptr(X), ptr(uv), ctypes.cast(k, ctypes.c_void_p), S, ptr(poses), ptr(n),
                                     current_stream(dev))
    check(rc, "isr_p3p_all_roots")
    return poses, n


def ransac_score(p3d, p2d, Kcam, Rt, ok, reperr: float, M_dev=None):
    import ctypes
    dev = require_cuda(p3d, p2d, Rt, ok)
    p3d, p2d, Rt = _f32c(p3d), _f32c(p2d), _f64c(Rt)
    cap, H = p3d.shape[0], Rt.numel() // 12
    M_dev = _m_dev(M_dev, dev, cap)
    n_inl = torch.empty(H, dtype=torch.int32, device=dev)
    best = torch.empty(1, dtype=torch.int32, device=dev)
    mask = torch.zeros((cap + 31) // 32, dtype=torch.int32, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_pnp_ransac_batch_workspace_bytes(cap, H, 1, _capi.FINAL_REFIT), "ransac")
    k = _kcam(Kcam)
    with torch.cuda.device(dev):
        rc = L.isr_ransac_score(ptr(p3d), ptr(p2d), ptr(M_dev), cap, ctypes.cast(k, ctypes.c_void_p),
                                ptr(Rt), ptr(ok.contiguous()), H, float(reperr), ptr(n_inl), ptr(best),
                                ptr(mask), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_ransac_score")
    return n_inl, best, mask


def pnp_refine(p3d, p2d, Kcam, Rt0, mask=None, iters: int = 10, M_dev=None):
    import ctypes
    dev = require_cuda(p3d, p2d, Rt0)
    p3d, p2d = _f32c(p3d), _f32c(p2d)
    cap = p3d.shape[0]
    M_dev = _m_dev(M_dev, dev, cap)
    Rt = _f64c(Rt0).clone().reshape(3, 4)
    L = lib()
    ws = workspace(dev, 1 << 20, "refine")
    k = _kcam(Kcam)
    with torch.cuda.device(dev):
        rc = L.isr_pnp_refine(ptr(p3d), ptr(p2d), ptr(M_dev), cap, ptr(mask), ctypes.cast(k, ctypes.c_void_p),
                              int(iters), ptr(Rt), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_pnp_refine")
    return Rt


@dataclass
class PnPResult:
    pose: torch.Tensor      # (3,4) f64 device
    inl_idx: torch.Tensor   # (cap,) i32 device, first n_inl valid
    n_inl: torch.Tensor     # (1,) i32 device
    status: torch.Tensor    # (1,) i32 device
    n_eval: torch.Tensor | None = None   # (1,) i32 device: hypotheses the staged loop scored (sequential: that ran)


@dataclass
class PnPBatchResult:
    pose: torch.Tensor      # (B,3,4) f64 device
    inl_idx: torch.Tensor   # (B,cap) i32 device, first n_inl[b] valid
    n_inl: torch.Tensor     # (B,) i32 device
    status: torch.Tensor    # (B,) i32 device
    n_eval: torch.Tensor | None = None   # (B,) i32 device: hypotheses the staged loop scored (sequential: that ran) per image


_LOOPS = {"staged": _capi.RANSAC_STAGED, "sequential": _capi.RANSAC_SEQUENTIAL}
_INLIERS = {"refit": _capi.INLIERS_REFIT, "ransac": _capi.INLIERS_RANSAC}
_FINALS = {"refit": _capi.FINAL_REFIT, "epnp": _capi.FINAL_EPNP}


def _loop_args(loop: str, inliers: str, stage0, final: str = "refit"):
    """(loop, stage0, inliers_mode, final_mode) of isr_pnp_ransac_batch; stage0 None = the default first stage (32)."""
    if loop not in _LOOPS:
        raise ValueError(f"loop={loop!r}: 'staged' or 'sequential'")
    if inliers not in _INLIERS:
        raise ValueError(f"inliers={inliers!r}: 'refit' or 'ransac'")
    if final not in _FINALS:
        raise ValueError(f"final={final!r}: 'refit' or 'epnp'")
    return _LOOPS[loop], 0 if stage0 is None else int(stage0), _INLIERS[inliers], _FINALS[final]


def _pnp_ransac(p3d, p2d, M_dev, Kcams, seeds, H, reperr, confidence, refine_iters, modes) -> PnPBatchResult:
    """isr_pnp_ransac_batch, the one body of pnp_ransac and pnp_ransac_batch: p3d (B, cap, 3), p2d (B, cap, 2) f32
    contiguous, M_dev (B,) i32 on the device; Kcams / seeds HOST pointers to (B, 9) f64 / (B,) u64; modes =
    _loop_args(...).  Every output stays on the device, nothing is pre-filled."""
    dev = p3d.device
    B, cap = p3d.shape[0], p3d.shape[1]
    pose = torch.empty((B, 3, 4), dtype=torch.float64, device=dev)
    inl = torch.empty((B, cap), dtype=torch.int32, device=dev)
    n_inl = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    n_eval = torch.empty(B, dtype=torch.int32, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_pnp_ransac_batch_workspace_bytes(cap, H, B, modes[3]), "ransac")
    with torch.cuda.device(dev), _timed("pnp_ransac", 30.0 * H * cap * B):
        rc = L.isr_pnp_ransac_batch(ptr(p3d), ptr(p2d), ptr(M_dev), cap, B, Kcams, int(H), seeds, float(reperr),
                                    float(confidence), int(refine_iters), ptr(pose), ptr(inl), ptr(n_inl), ptr(status),
                                    ptr(n_eval), ptr(ws), ws.numel(), current_stream(dev), *modes)
    check(rc, "isr_pnp_ransac_batch")
    return PnPBatchResult(pose, inl, n_inl, status, n_eval)


def pnp_ransac(p3d, p2d, Kcam, H: int = 500, reperr: float = 2.0, seed: int = 0,
               refine_iters: int = 10, M_dev=None, confidence: float = 0.99, loop: str = "staged",
               inliers: str = "refit", stage0: int | None = None, final: str = "refit") -> PnPResult:
    """pnp_ransac_batch of one image, fully asynchronous: every output stays on the device.  confidence: cv2's
    solvePnPRansac parameter (default 0.99, what the reference's call uses); >= 1 scores every hypothesis (staged loop).
    loop="staged" (default): scoring stops at a stage boundary 32 (2^k - 1) once the confidence is reached, the best of
    every scored hypothesis wins.  loop="sequential": OpenCV's loop — hypothesis h runs while h < niters, niters updated
    from the best count so far; n_eval = how many ran; the result does not depend on stage0 (the first scoring stage, a
    multiple of 32 or >= H; None = 32).  inliers="refit" (default): the inliers of the returned, refitted pose;
    "ransac": the winning hypothesis' consensus set, as cv2 reports it.  final="refit" (default): the pose is the
    Gauss-Newton refit with its local-optimisation round; "epnp": cv2's final solve, EPnP over the winner's consensus set
    (refine_iters unused; a non-finite EPnP pose gives status 0)."""
    modes = _loop_args(loop, inliers, stage0, final)
    dev = require_cuda(p3d, p2d)
    p3d, p2d = _f32c(p3d), _f32c(p2d)
    r = _pnp_ransac(p3d[None], p2d[None], _m_dev(M_dev, dev, p3d.shape[0]), ctypes.cast(_kcam(Kcam), ctypes.c_void_p),
                    ctypes.byref(ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF)), H, reperr, confidence, refine_iters, modes)
    return PnPResult(r.pose[0], r.inl_idx[0], r.n_inl, r.status, r.n_eval)


def ransac_seq_host(n_inl, ok, M: int, confidence: float = 0.99) -> tuple[int, int]:
    """isr_ransac_seq_host: OpenCV's sequential RANSAC loop over host arrays of counts n_inl (H,) and model flags ok (H,),
    from the header the kernels use (no device) -> (winner, n_eval); winner -1: no hypothesis with more than 3 inliers."""
    c = np.ascontiguousarray(n_inl, dtype=np.int32)
    o = np.ascontiguousarray(ok, dtype=np.uint8)
    if c.ndim != 1 or o.shape != c.shape:
        raise ValueError(f"ransac_seq_host: n_inl {c.shape} / ok {o.shape} must be (H,)")
    w, n = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().isr_ransac_seq_host(c.ctypes.data_as(ctypes.c_void_p), o.ctypes.data_as(ctypes.c_void_p), c.shape[0], int(M),
                                    float(confidence), ctypes.byref(w), ctypes.byref(n)), "isr_ransac_seq_host")
    return int(w.value), int(n.value)


def epnp_batch(p3d, p2d, Kcams, M_dev=None, mask=None):
    """isr_epnp_batch: EPnP (csrc/epnp.hpp) on the device.  p3d (B, cap, 3), p2d (B, cap, 2) (or one image, (cap, 3) /
    (cap, 2)); M_dev (B,) i32 (None: cap); mask (B, ceil(cap / 32)) u32 words as int32 (None: every point below M);
    Kcams one 3x3 or (B, 3, 3) host array -> Rt (B, 3, 4) f64, rep_err (B, 3) f64, chosen (B,) i32 (1..3; 0 and a NaN pose:
    fewer than 4 masked points), all on the device.  Image b's result equals epnp_host on image b's points, bit for bit."""
    import ctypes
    dev = require_cuda(p3d, p2d, M_dev, mask)
    p3d, p2d = _f32c(p3d), _f32c(p2d)
    if p3d.ndim == 2:
        p3d, p2d = p3d[None], p2d[None]
    B, cap = p3d.shape[0], p3d.shape[1]
    if tuple(p2d.shape) != (B, cap, 2) or p3d.shape[2] != 3:
        raise ValueError(f"epnp_batch: p3d {tuple(p3d.shape)} / p2d {tuple(p2d.shape)} must be (B,cap,3)/(B,cap,2)")
    if M_dev is None:
        M_dev = torch.full((B,), cap, dtype=torch.int32, device=dev)
    if mask is not None:
        mask = mask.contiguous()
        if mask.dtype != torch.int32 or tuple(mask.shape) != (B, (cap + 31) // 32):
            raise ValueError(f"epnp_batch: mask must be a ({B}, {(cap + 31) // 32}) int32 tensor")
    K = np.asarray(Kcams, dtype=np.float64)
    K = np.ascontiguousarray(np.broadcast_to(K.reshape(-1, 3, 3), (B, 3, 3)) if K.size == 9 else K.reshape(B, 3, 3))
    Rt = torch.empty((B, 3, 4), dtype=torch.float64, device=dev)
    err = torch.empty((B, 3), dtype=torch.float64, device=dev)
    chosen = torch.empty(B, dtype=torch.int32, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_epnp_batch_workspace_bytes(cap, B), "epnp")
    with torch.cuda.device(dev):
        rc = L.isr_epnp_batch(ptr(p3d), ptr(p2d), ptr(M_dev.contiguous()), cap, B, ptr(mask), K.ctypes.data_as(ctypes.c_void_p),
                              ptr(Rt), ptr(err), ptr(chosen), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_epnp_batch")
    return Rt, err, chosen


def epnp_host(p3d, p2d, Kcam, mask=None):
    """isr_epnp_host: the same solver as host code, the device's reduction shape replayed.  p3d (M, 3), p2d (M, 2) (cast to
    f32), mask (ceil(M / 32),) u32 words or None -> (Rt (3, 4) f64, rep_err (3,) f64, chosen 1..3)."""
    a = np.ascontiguousarray(np.asarray(p3d), dtype=np.float32)
    b = np.ascontiguousarray(np.asarray(p2d), dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3 or b.shape != (a.shape[0], 2):
        raise ValueError(f"epnp_host: p3d {a.shape} / p2d {b.shape} must be (M,3)/(M,2)")
    M = a.shape[0]
    mk = None
    if mask is not None:
        mk = np.ascontiguousarray(np.asarray(mask).astype(np.uint32, copy=False))
        if mk.shape != ((M + 31) // 32,):
            raise ValueError(f"epnp_host: mask {mk.shape} must be ({(M + 31) // 32},)")
    k = np.ascontiguousarray(np.asarray(Kcam, dtype=np.float64).reshape(9))
    Rt = np.empty(12, np.float64)
    err = np.empty(3, np.float64)
    ch = ctypes.c_int32(0)
    vp = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_epnp_host(vp(a), vp(b), vp(mk), M, vp(k), vp(Rt), vp(err), ctypes.byref(ch)), "isr_epnp_host")
    return Rt.reshape(3, 4), err, int(ch.value)


def epnp_jacobi_host(A):
    """isr_epnp_jacobi_host: EPnP's Jacobi eigen-decomposition of a symmetric (n, n), n <= 12 -> (eigenvalues ascending,
    eigenvectors as columns)."""
    a = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
    n = a.shape[0]
    if a.shape != (n, n):
        raise ValueError(f"epnp_jacobi_host: A {a.shape} must be square")
    w = np.empty(n, np.float64)
    V = np.empty((n, n), np.float64)
    check(lib().isr_epnp_jacobi_host(a.ctypes.data_as(ctypes.c_void_p), n, w.ctypes.data_as(ctypes.c_void_p),
                                     V.ctypes.data_as(ctypes.c_void_p)), "isr_epnp_jacobi_host")
    return w, V


# ------------------------------------------------------------------ the per-group (batched) chain
def select_top_batch(logp: torch.Tensor, frac: float = 0.8, min_n: int = 500, n_dev: torch.Tensor | None = None,
                     digit_hist: torch.Tensor | None = None):
    """isr_select_top_batch: logp (B, P) -> keep (B, P) i32 (first M[b] valid, ascending), M (B,) i32,
    thr (B,) f32.  One chain of ten launches for the whole group; outputs are not pre-filled.
    digit_hist (B, 2048) i32: the first histogram as corr_argmax(..., rows_per_image=P, n_rows=n_dev) left it for these
    values (isr_select_top_batch_digits: nine launches, one read of logp less, the same results)."""
    dev = require_cuda(logp, n_dev, digit_hist)
    logp = _f32c(logp)
    B, P = logp.shape
    keep = torch.empty((B, P), dtype=torch.int32, device=dev)
    M_dev = torch.empty(B, dtype=torch.int32, device=dev)
    thr = torch.empty(B, dtype=torch.float32, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_select_top_batch_workspace_bytes(P, B), "select")
    if digit_hist is not None and (digit_hist.dtype != torch.int32 or tuple(digit_hist.shape) != (B, 2048) or not digit_hist.is_contiguous()):
        raise ValueError(f"select_top_batch: digit_hist must be a contiguous ({B}, 2048) int32 tensor")
    with torch.cuda.device(dev), _timed("select_top", 4.0 * P * B):
        if digit_hist is None:
            rc = L.isr_select_top_batch(ptr(logp), P, B, ptr(n_dev), float(frac), int(min_n), ptr(keep), ptr(M_dev),
                                        ptr(thr), ptr(ws), ws.numel(), current_stream(dev))
        else:
            rc = L.isr_select_top_batch_digits(ptr(logp), P, B, ptr(n_dev), float(frac), int(min_n), ptr(digit_hist), ptr(keep),
                                               ptr(M_dev), ptr(thr), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_select_top_batch")
    return keep, M_dev, thr


def gather_corr_batch(idx, keep, M_dev, pts, pix_xy):
    """isr_gather_corr_batch: idx, keep (B, P); pix_xy (P, 2) shared or (B, P, 2) -> p3d (B, P, 3), p2d (B, P, 2)."""
    dev = require_cuda(idx, keep, M_dev, pts, pix_xy)
    pts, pix_xy = _f32c(pts), _f32c(pix_xy)
    B, P = keep.shape
    shared = pix_xy.ndim == 2
    if tuple(pix_xy.shape) != ((P, 2) if shared else (B, P, 2)) or tuple(idx.shape) != (B, P):
        raise ValueError(f"gather_corr_batch: idx {tuple(idx.shape)} / keep {tuple(keep.shape)} / pix_xy {tuple(pix_xy.shape)}")
    p3d = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
    p2d = torch.empty((B, P, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib().isr_gather_corr_batch(ptr(idx.contiguous()), ptr(keep), ptr(M_dev), P, B, ptr(pts), pts.shape[0],
                                         ptr(pix_xy), int(shared), ptr(p3d), ptr(p2d), current_stream(dev))
    check(rc, "isr_gather_corr_batch")
    return p3d, p2d


def pnp_ransac_batch(p3d, p2d, Kcams, M_dev, H: int = 500, reperr: float = 2.0, seeds=None,
                     refine_iters: int = 10, confidence: float = 0.99, loop: str = "staged", inliers: str = "refit",
                     stage0: int | None = None, final: str = "refit") -> PnPBatchResult:
    """isr_pnp_ransac_batch: p3d (B, cap, 3), p2d (B, cap, 2), M_dev (B,) i32; Kcams one 3x3 or (B, 3, 3)
    host array; seeds B ints.  Every output stays on the device, nothing is pre-filled.  loop / inliers / stage0 / final:
    as pnp_ransac; image b's outputs equal pnp_ransac's on image b alone."""
    modes = _loop_args(loop, inliers, stage0, final)
    dev = require_cuda(p3d, p2d, M_dev)
    p3d, p2d = _f32c(p3d), _f32c(p2d)
    B = p3d.shape[0]
    K = np.asarray(Kcams, dtype=np.float64)
    K = np.ascontiguousarray(np.broadcast_to(K.reshape(-1, 3, 3), (B, 3, 3)) if K.size == 9 else K.reshape(B, 3, 3))
    sd = np.ascontiguousarray(np.asarray([0] * B if seeds is None else [int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds],
                                         dtype=np.uint64))
    if sd.shape != (B,):
        raise ValueError("pnp_ransac_batch: one seed per image")
    return _pnp_ransac(p3d, p2d, M_dev, K.ctypes.data_as(ctypes.c_void_p), sd.ctypes.data_as(ctypes.c_void_p), H, reperr,
                       confidence, refine_iters, modes)


def add_metric(verts: torch.Tensor, Ta: torch.Tensor | None, Tb: torch.Tensor | None) -> torch.Tensor:
    """isr_add_metric: (B,) f64 mean vertex distance between poses Ta[b] and Tb[b]."""
    dev = require_cuda(verts, Ta, Tb)
    verts, Ta, Tb = _f32c(verts), _f64c(Ta), _f64c(Tb)
    B = max([1] + [T.numel() // 12 for T in (Ta, Tb) if T is not None])
    out = torch.empty(B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib().isr_add_metric(ptr(verts), verts.shape[0], ptr(Ta), ptr(Tb), B, ptr(out), current_stream(dev))
    check(rc, "isr_add_metric")
    return out


def refine_objective_batch(X_all: torch.Tensor, keys_all: torch.Tensor, offs, query_imgs: torch.Tensor,
                           denom_imgs: torch.Tensor, K: torch.Tensor, item_img: torch.Tensor, Rt: torch.Tensor, nout: int = 4,
                           interpolation: int = 0, *, offs_dev: torch.Tensor | None = None, n_items: int | None = None,
                           out: torch.Tensor | None = None) -> torch.Tensor:
    """isr_refine_objective_batch: (n_items, nout) f64, row i = the refine objective of image item_img[i] at pose Rt[i]
    (nout 4: score, d/dt; 13: + d/dR), the bits of isr_refine_objective(_full) on that item alone.
    X_all (sum N, 3), keys_all (sum N, e) f32; offs the n_img + 1 row offsets on the HOST (sequence or array; offs_dev its
    device copy, made here when not given); query_imgs (n_img, res, res, e), denom_imgs (n_img, res, res) f32; K (n_img, 9)
    f64; item_img (>= n_items,) i32; Rt (>= n_items, 12) f64 — device tensors.  n_items defaults to len(item_img)."""
    dev = require_cuda(X_all, keys_all, query_imgs, denom_imgs, K, item_img, Rt, offs_dev)
    offs_h = np.ascontiguousarray(np.asarray(offs, dtype=np.int32))
    n_img = offs_h.shape[0] - 1
    n = item_img.shape[0] if n_items is None else int(n_items)
    for name, t, dt in (("X_all", X_all, torch.float32), ("keys_all", keys_all, torch.float32),
                        ("query_imgs", query_imgs, torch.float32), ("denom_imgs", denom_imgs, torch.float32),
                        ("K", K, torch.float64), ("item_img", item_img, torch.int32), ("Rt", Rt, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"refine_objective_batch: {name} must be a contiguous {dt} tensor")
    res, e = query_imgs.shape[1], query_imgs.shape[-1]
    if (query_imgs.shape != (n_img, res, res, e) or denom_imgs.shape != (n_img, res, res) or K.numel() != 9 * n_img
            or keys_all.shape != (X_all.shape[0], e) or X_all.shape[1:] != (3,) or n_img < 1
            or int(offs_h[-1]) != X_all.shape[0] or item_img.shape[0] < n or Rt.numel() < 12 * n):
        raise ValueError(f"refine_objective_batch: X_all {tuple(X_all.shape)} keys_all {tuple(keys_all.shape)} offs "
                         f"{offs_h.tolist()[:4]}... query_imgs {tuple(query_imgs.shape)} denom_imgs {tuple(denom_imgs.shape)} "
                         f"K {tuple(K.shape)} item_img {tuple(item_img.shape)} Rt {tuple(Rt.shape)} n_items {n}")
    if offs_dev is None:
        offs_dev = torch.from_numpy(offs_h).to(dev)
    if out is None:
        out = torch.empty((n, nout), dtype=torch.float64, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_refine_objective_batch_workspace_bytes(n), "refine_obj_batch")
    with torch.cuda.device(dev), _timed("refine_objective_batch", 0.0):
        rc = L.isr_refine_objective_batch(ptr(X_all), ptr(keys_all), offs_h.ctypes.data_as(ctypes.c_void_p), ptr(offs_dev),
                                          n_img, e, ptr(query_imgs), ptr(denom_imgs), res, int(interpolation), ptr(K),
                                          ptr(item_img), ptr(Rt), n, ptr(out), int(nout), ptr(ws), ws.numel(),
                                          current_stream(dev))
    check(rc, "isr_refine_objective_batch")
    return out


def refine_bfgs_batch(X_all: torch.Tensor, keys_all: torch.Tensor, offs, query_imgs: torch.Tensor, denom_imgs: torch.Tensor,
                      K: torch.Tensor, item_img: torch.Tensor, R: torch.Tensor, t0: torch.Tensor, interpolation: int = 0, *,
                      gtol: float = 1e-5, maxiter: int | None = None, max_rounds: int = 100_000,
                      offs_dev: torch.Tensor | None = None) -> dict:
    """isr_refine_bfgs_batch: refine_pose's scipy BFGS over t for n_items (image item_img[i], fixed R[i], start t0[i]), run on
    the device.  The image arguments are refine_objective_batch's; R (n, 3, 3) or (n, 9), t0 (n, 3) f64, item_img (n,) i32 —
    device tensors.  maxiter defaults to scipy's 200 * 6.  Returns {t (n, 3), fun (n,) f64, nit, nfev, status (n,) i32 — device
    tensors; rounds, launches — ints}.  status: scipy's (0 .. 3) or 4 = max_rounds ran out while the item was live."""
    dev = require_cuda(X_all, keys_all, query_imgs, denom_imgs, K, item_img, R, t0, offs_dev)
    offs_h = np.ascontiguousarray(np.asarray(offs, dtype=np.int32))
    n_img = offs_h.shape[0] - 1
    n = item_img.shape[0]
    for name, t, dt in (("X_all", X_all, torch.float32), ("keys_all", keys_all, torch.float32),
                        ("query_imgs", query_imgs, torch.float32), ("denom_imgs", denom_imgs, torch.float32),
                        ("K", K, torch.float64), ("item_img", item_img, torch.int32), ("R", R, torch.float64),
                        ("t0", t0, torch.float64)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"refine_bfgs_batch: {name} must be a contiguous {dt} tensor")
    res, e = query_imgs.shape[1], query_imgs.shape[-1]
    if (query_imgs.shape != (n_img, res, res, e) or denom_imgs.shape != (n_img, res, res) or K.numel() != 9 * n_img
            or keys_all.shape != (X_all.shape[0], e) or X_all.shape[1:] != (3,) or n_img < 1
            or int(offs_h[-1]) != X_all.shape[0] or R.numel() != 9 * n or t0.numel() != 3 * n):
        raise ValueError(f"refine_bfgs_batch: X_all {tuple(X_all.shape)} keys_all {tuple(keys_all.shape)} offs "
                         f"{offs_h.tolist()[:4]}... query_imgs {tuple(query_imgs.shape)} denom_imgs {tuple(denom_imgs.shape)} "
                         f"K {tuple(K.shape)} item_img {tuple(item_img.shape)} R {tuple(R.shape)} t0 {tuple(t0.shape)}")
    if offs_dev is None:
        offs_dev = torch.from_numpy(offs_h).to(dev)
    maxiter = 200 * 6 if maxiter is None else int(maxiter)
    t_out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    fun = torch.empty(n, dtype=torch.float64, device=dev)
    info = torch.empty((3, n), dtype=torch.int32, device=dev)
    stats = (ctypes.c_int32 * 2)()
    L = lib()
    ws = workspace(dev, L.isr_refine_bfgs_batch_workspace_bytes(n), "refine_bfgs")
    with torch.cuda.device(dev), _timed("refine_bfgs_batch", 0.0):
        rc = L.isr_refine_bfgs_batch(ptr(X_all), ptr(keys_all), offs_h.ctypes.data_as(ctypes.c_void_p), ptr(offs_dev), n_img,
                                     e, ptr(query_imgs), ptr(denom_imgs), res, int(interpolation), ptr(K), ptr(item_img),
                                     ptr(R), ptr(t0), n, float(gtol), maxiter, int(max_rounds), ptr(t_out), ptr(fun),
                                     ptr(info[0]), ptr(info[1]), ptr(info[2]), ctypes.cast(stats, ctypes.c_void_p), ptr(ws),
                                     ws.numel(), current_stream(dev))
    check(rc, "isr_refine_bfgs_batch")
    return {"t": t_out, "fun": fun, "nit": info[0], "nfev": info[1], "status": info[2], "rounds": int(stats[0]),
            "launches": int(stats[1])}


def corr_logsoftmax(queries: torch.Tensor, keys: torch.Tensor) -> torch.Tensor:
    """isr_corr_logsoftmax: the full (P,N) f32 log-softmax matrix (small P only: it is written out)."""
    dev = require_cuda(queries, keys)
    if queries.dtype == torch.bfloat16 and keys.dtype == torch.bfloat16:
        dtype = _capi.DTYPE_BF16
    else:
        dtype = _capi.DTYPE_F32
        queries, keys = queries.to(torch.float32), keys.to(torch.float32)
    q, k = queries.contiguous(), keys.contiguous()
    P, D = q.shape
    N = k.shape[0]
    out = torch.empty((P, N), dtype=torch.float32, device=dev)
    L = lib()
    ws = workspace(dev, L.isr_corr_logsoftmax_workspace_bytes(P, N, D, dtype), "corr_lsm")
    with torch.cuda.device(dev):
        rc = L.isr_corr_logsoftmax(ptr(q), ptr(k), P, N, D, D, D, dtype, ptr(out), N, ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_corr_logsoftmax")
    return out


def render_state_words(h: int, w: int) -> int:
    """4-byte words of one frame-buffer block of isr_render_coords_batch: h*w*4 colour | h*w depth | 4 counters."""
    return 5 * h * w + 4


def render_coords_batch(verts: torch.Tensor, faces: torch.Tensor, K: torch.Tensor, Rt: torch.Tensor, h: int, w: int,
                        offset: torch.Tensor, scale: float, near: float = 10.0, far: float = 10000.0, clear: bool = True,
                        state: torch.Tensor | None = None) -> torch.Tensor:
    """isr_render_coords_batch: the mesh verts (V,3) f32, faces (F,3) i32 drawn at B poses Rt (B,12) f64 with cameras K (B,9)
    f64 into `state` (B, 5*h*w+4) f32 (allocated when None; required for clear=False, which draws on top of it).
    Returns `state`: [:, :4*h*w] is the (h,w,4) colour, [:, 4*h*w:5*h*w] the depth, the last 4 words the i32 counters."""
    dev = require_cuda(verts, faces, K, Rt, offset, state)
    if (verts.dtype != torch.float32 or faces.dtype != torch.int32 or offset.dtype != torch.float32 or K.dtype != torch.float64
            or Rt.dtype != torch.float64 or not all(t.is_contiguous() for t in (verts, faces, K, Rt, offset))):
        raise ValueError("render_coords_batch: contiguous verts f32, faces i32, offset f32, K f64, Rt f64")
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3 or offset.numel() != 3:
        raise ValueError(f"render_coords_batch: verts {tuple(verts.shape)} (V,3), faces {tuple(faces.shape)} (F,3), offset (3)")
    B = Rt.numel() // 12
    if Rt.numel() != B * 12 or K.numel() != B * 9:
        raise ValueError(f"render_coords_batch: Rt {tuple(Rt.shape)} (B,12) and K {tuple(K.shape)} (B,9) disagree")
    words = render_state_words(h, w)
    if state is None:
        if not clear:
            raise ValueError("render_coords_batch: clear=False draws on top of `state`, which must be given")
        state = torch.empty((B, words), dtype=torch.float32, device=dev)
    elif state.dtype != torch.float32 or state.numel() != B * words or not state.is_contiguous():
        raise ValueError(f"render_coords_batch: state must be contiguous (B, {words}) float32, got {tuple(state.shape)} {state.dtype}")
    L = lib()
    V, F = verts.shape[0], faces.shape[0]
    ws = workspace(dev, L.isr_render_coords_batch_workspace_bytes(V, F, h, w, B), "render")
    with torch.cuda.device(dev), _timed("render_coords", float(B) * F):
        rc = L.isr_render_coords_batch(ptr(verts), V, ptr(faces), F, ptr(K), ptr(Rt), B, h, w, ptr(offset), float(scale),
                                       float(near), float(far), 1 if clear else 0, ptr(state), ptr(ws), ws.numel(),
                                       current_stream(dev))
    check(rc, "isr_render_coords_batch")
    return state


def render_coords_host(verts, faces, K, Rt, h: int, w: int, offset, scale: float, near: float = 10.0, far: float = 10000.0,
                       clear: bool = True, state=None):
    """isr_render_coords_host: the same rasteriser as host code, one item.  NumPy in (verts (V,3) cast to f32, faces (F,3) to
    i32, K (3,3), Rt (3,4) or (12,)), -> state (5*h*w+4,) f32 (`state` is drawn on, in place, when given)."""
    v = np.ascontiguousarray(verts, np.float32)
    f = np.ascontiguousarray(faces, np.int32)
    k = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
    rt = np.ascontiguousarray(np.asarray(Rt, np.float64).reshape(12))
    o = np.ascontiguousarray(np.asarray(offset, np.float32).reshape(3))
    words = render_state_words(h, w)
    if state is None:
        if not clear:
            raise ValueError("render_coords_host: clear=False draws on top of `state`, which must be given")
        state = np.empty(words, np.float32)
    elif state.dtype != np.float32 or state.size != words or not state.flags.c_contiguous:
        raise ValueError(f"render_coords_host: state must be contiguous ({words},) float32")
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_render_coords_host(vp(v), v.shape[0], vp(f), f.shape[0], vp(k), vp(rt), h, w, vp(o), float(scale),
                                       float(near), float(far), 1 if clear else 0, vp(state)), "isr_render_coords_host")
    return state


def field_flops(widths) -> float:
    """Multiply-adds x 2 of one point through a field of these widths."""
    return 2.0 * sum(int(a) * int(b) for a, b in zip(widths[:-1], widths[1:]))


def _points_n3(name: str, points: torch.Tensor) -> int:
    if points.dtype != torch.float32 or points.ndim != 2 or points.shape[1] != 3 or not points.is_contiguous():
        raise ValueError(f"{name}: points must be contiguous (N,3) float32, got {tuple(points.shape)} {points.dtype}")
    return points.shape[0]


def _field_args(pack: torch.Tensor, widths, n_layers: int):
    w = (ctypes.c_int32 * len(widths))(*[int(v) for v in widths])
    return ptr(pack), pack.numel() * pack.element_size(), n_layers, ctypes.cast(w, ctypes.c_void_p), w      # w: kept alive by the caller


def field_eval(pack: torch.Tensor, widths, points: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """isr_field_eval: points (N,3) f32 through the packed field (`pack`: the device copy of isr_field_pack's bytes for these
    `widths`, fields.KeyField builds it) -> out (N, ld) f32, ld >= widths[-1] (allocated (N, widths[-1]) when None); only
    columns < widths[-1] are written."""
    dev = require_cuda(pack, points, out)
    N, o = _points_n3("field_eval", points), int(widths[-1])
    if out is None:
        out = torch.empty((N, o), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.ndim != 2 or out.shape[0] != N or not out.is_contiguous():
        raise ValueError(f"field_eval: out must be contiguous ({N}, >= {o}) float32, got {tuple(out.shape)} {out.dtype}")
    pk, nbytes, nl, wp, _keep = _field_args(pack, widths, len(widths) - 1)
    with torch.cuda.device(dev), _timed("field_eval", N * field_flops(widths)):
        rc = lib().isr_field_eval(pk, nbytes, nl, wp, ptr(points) if N else None, N, ptr(out) if N else None, out.shape[1],
                                  current_stream(dev))
    check(rc, "isr_field_eval")
    return out


def density_flops(widths, H: int) -> float:
    """Multiply-adds x 2 of one point through a density field: 6H -> widths... -> 1."""
    w = [6 * int(H)] + [int(v) for v in widths] + [1]
    return 2.0 * sum(a * b for a, b in zip(w[:-1], w[1:]))


def density_eval(pack: torch.Tensor, widths, H: int, points: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """isr_density_eval: points (N,3) f32 through the packed density field (`pack`: the device copy of isr_density_pack's
    bytes for these hidden `widths` and `H` frequencies, fields.DensityField builds it) -> out (N,) f32."""
    dev = require_cuda(pack, points, out)
    N = _points_n3("density_eval", points)
    if out is None:
        out = torch.empty((N,), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.shape != (N,) or not out.is_contiguous():
        raise ValueError(f"density_eval: out must be contiguous ({N},) float32, got {tuple(out.shape)} {out.dtype}")
    pk, nbytes, nh, wp, _keep = _field_args(pack, widths, len(widths))
    with torch.cuda.device(dev), _timed("density_eval", N * density_flops(widths, H)):
        rc = lib().isr_density_eval(pk, nbytes, nh, wp, int(H), ptr(points) if N else None, N, ptr(out) if N else None,
                                    current_stream(dev))
    check(rc, "isr_density_eval")
    return out


MARCH_DIRECTIONS = {"front": 0, "back": 1, "both": 2}


def march_direction(direction: str) -> int:
    """ISR_MARCH_* of include/isr_density_dir.h for "front", "back" or "both"."""
    if direction not in MARCH_DIRECTIONS:
        raise ValueError(f"density_march: direction = {direction!r} (front, back or both)")
    return MARCH_DIRECTIONS[direction]


def _ray_bundle(name: str, origins, directions, lengths, threshold) -> tuple[int, int, float]:
    """The checks of a bundle origins (N,3), directions (N,3), lengths (N,P) and its threshold -> (N, P, threshold)."""
    for what, t, cols in (("origins", origins, 3), ("directions", directions, 3), ("lengths", lengths, None)):
        if t.dtype != torch.float32 or t.ndim != 2 or (cols and t.shape[1] != cols) or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be contiguous 2-d float32, got {tuple(t.shape)} {t.dtype}")
    N, P = lengths.shape
    if origins.shape[0] != N or directions.shape[0] != N:
        raise ValueError(f"{name}: {origins.shape[0]} origins, {directions.shape[0]} directions, {N} rows of lengths")
    if P < 1:
        raise ValueError(f"{name}: P < 1")
    thr = float(threshold)
    if thr != thr:
        raise ValueError(f"{name}: threshold is NaN")
    return N, P, thr


def density_march(pack: torch.Tensor, widths, H: int, origins: torch.Tensor, directions: torch.Tensor, lengths: torch.Tensor,
                  threshold: float = 0.2, want_densities: bool = False, want_weights: bool = False, direction: str = "front"):
    """isr_density_march: origins (N,3), directions (N,3), lengths (N,P) f32 -> (points (N,3) f32, depth (N,) f32,
    hit (N,) int32, densities (N,P) f32 or None, weights (N,P) f32 or None).  threshold >= 0: the weight is one at the first
    density above it (the reference's thresholdMode); threshold < 0: emission-absorption weights.
    direction (isr_density_march_dir): "front" is the above; "back" the same outputs for the march from the far end of the
    ray (one at the LAST density above the threshold: the exit point, prenBack.py:378-381); "both" gives points (2,N,3),
    depth (2,N), hit (2,N), front then back, and weights (N,2P), a ray's front weights then its back weights."""
    dev = require_cuda(pack, origins, directions, lengths)
    N, P, thr = _ray_bundle("density_march", origins, directions, lengths, threshold)
    way = march_direction(direction)
    lead = (2, N) if way == 2 else (N,)
    f32 = dict(dtype=torch.float32, device=dev)
    points, depth = torch.empty((*lead, 3), **f32), torch.empty(lead, **f32)
    hit = torch.empty(lead, dtype=torch.int32, device=dev)
    dens = torch.empty((N, P), **f32) if want_densities else None
    wts = torch.empty((N, 2 * P if way == 2 else P), **f32) if want_weights else None
    pk, nbytes, nh, wp, _keep = _field_args(pack, widths, len(widths))
    work = float(N) * P * density_flops(widths, H)
    if way == 0:
        with torch.cuda.device(dev), _timed("density_march", work):
            rc = lib().isr_density_march(pk, nbytes, nh, wp, int(H), ptr(origins), ptr(directions), ptr(lengths), N, P, thr,
                                         ptr(dens), ptr(wts), ptr(depth), ptr(points), ptr(hit), current_stream(dev))
        check(rc, "isr_density_march")
    else:
        with torch.cuda.device(dev), _timed("density_march_" + direction, work):
            rc = lib().isr_density_march_dir(pk, nbytes, nh, wp, int(H), ptr(origins), ptr(directions), ptr(lengths), N, P, thr,
                                             way, ptr(dens), ptr(wts), ptr(depth), ptr(points), ptr(hit), current_stream(dev))
        check(rc, "isr_density_march_dir")
    return points, depth, hit, dens, wts


def density_march_given_host(lengths, rho, threshold: float, direction: str = "front"):
    """isr_density_march_given_host: the march alone of given densities, host code, NumPy (N,P), (N,P) -> (weights, depth,
    hit) shaped as density_march shapes them for `direction`.  For tests."""
    ln, r = np.ascontiguousarray(lengths, np.float32), np.ascontiguousarray(rho, np.float32)
    if ln.ndim != 2 or ln.shape != r.shape:
        raise ValueError(f"density_march_given_host: lengths {ln.shape}, rho {r.shape}")
    N, P = ln.shape
    way = march_direction(direction)
    lead = (2, N) if way == 2 else (N,)
    wts, depth, hit = np.empty((N, 2 * P if way == 2 else P), np.float32), np.empty(lead, np.float32), np.empty(lead, np.int32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_density_march_given_host(hp(ln), hp(r), N, P, float(threshold), way, hp(wts), hp(depth), hp(hit)),
          "isr_density_march_given_host")
    return wts, depth, hit


def radiance_flops(widths, H: int, Wc: int, C: int) -> float:
    """Multiply-adds x 2 of one point through a radiance field: the density field's and the colour head's trunk part
    (the direction's 6H x Wc block is per ray)."""
    return density_flops(widths, H) + 2.0 * (int(widths[-1]) * int(Wc) + int(Wc) * int(C))


def radiance_workspace_bytes(N: int, Wc: int) -> int:
    """isr_radiance_workspace_bytes: the device workspace radiance_render needs for N rays."""
    return int(lib().isr_radiance_workspace_bytes(int(N), int(Wc)))


def radiance_render(pack: torch.Tensor, widths, H: int, Wc: int, C: int, origins: torch.Tensor, directions: torch.Tensor,
                    lengths: torch.Tensor, threshold: float = -1.0, want_weights: bool = False, want_densities: bool = False,
                    want_colours: bool = False, workspace: torch.Tensor | None = None):
    """isr_radiance_render: origins (N,3), directions (N,3), lengths (N,P) f32 through the packed radiance field (`pack`:
    the device copy of isr_radiance_pack's bytes, fields.RadianceField builds it) -> dict of image (N, C+1) [features |
    opacity], depth (N,), points (N,3), hit (N,) int32 and weights (N,P), densities (N,P), colours (N,P,C) or None.
    threshold >= 0 is the reference's thresholdMode, a negative one the emission-absorption weights.  workspace: a
    contiguous device tensor of at least radiance_workspace_bytes(N, Wc) bytes to reuse (allocated when None)."""
    dev = require_cuda(pack, origins, directions, lengths, workspace)
    N, P, thr = _ray_bundle("radiance_render", origins, directions, lengths, threshold)
    Wc, C = int(Wc), int(C)
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(image=torch.empty((N, C + 1), **f32), depth=torch.empty((N,), **f32), points=torch.empty((N, 3), **f32),
               hit=torch.empty((N,), dtype=torch.int32, device=dev),
               weights=torch.empty((N, P), **f32) if want_weights else None,
               densities=torch.empty((N, P), **f32) if want_densities else None,
               colours=torch.empty((N, P, C), **f32) if want_colours else None)
    need = radiance_workspace_bytes(N, Wc) if N else 0
    if workspace is None:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    elif not workspace.is_contiguous():
        raise ValueError("radiance_render: the workspace must be contiguous")
    pk, nbytes, nh, wp, _keep = _field_args(pack, widths, len(widths))
    with torch.cuda.device(dev), _timed("radiance_render", float(N) * P * radiance_flops(widths, H, Wc, C)):
        rc = lib().isr_radiance_render(pk, nbytes, nh, wp, int(H), Wc, C, ptr(origins), ptr(directions), ptr(lengths), N, P, thr,
                                       ptr(out["image"]), ptr(out["depth"]), ptr(out["points"]), ptr(out["hit"]),
                                       ptr(out["weights"]), ptr(out["densities"]), ptr(out["colours"]), ptr(workspace),
                                       workspace.numel() * workspace.element_size(), current_stream(dev))
    check(rc, "isr_radiance_render")
    return out


def ea_march(densities: torch.Tensor, features: torch.Tensor, threshold: float = -1.0, want_weights: bool = True):
    """isr_ea_march: densities (N,P), features (N,P,F) f32 -> (image (N, F+1) [features | opacity], weights (N,P) or None):
    the emission-absorption march of pren.py:338-369 (threshold >= 0: thresholdMode) over tensors the caller has."""
    dev = require_cuda(densities, features)
    if (densities.dtype != torch.float32 or features.dtype != torch.float32 or densities.ndim != 2 or features.ndim != 3
            or features.shape[:2] != densities.shape or not densities.is_contiguous() or not features.is_contiguous()):
        raise ValueError(f"ea_march: densities {tuple(densities.shape)} {densities.dtype} and features {tuple(features.shape)} "
                         f"{features.dtype} must be contiguous float32 (N,P) and (N,P,F)")
    N, P, F = features.shape
    if P < 1 or F < 1:
        raise ValueError("ea_march: P < 1 or F < 1")
    thr = float(threshold)
    if thr != thr:
        raise ValueError("ea_march: threshold is NaN")
    image = torch.empty((N, F + 1), dtype=torch.float32, device=dev)
    wts = torch.empty((N, P), dtype=torch.float32, device=dev) if want_weights else None
    with torch.cuda.device(dev), _timed("ea_march", 2.0 * N * P * F):
        rc = lib().isr_ea_march(ptr(densities), ptr(features), N, P, F, thr, ptr(image), ptr(wts), current_stream(dev))
    check(rc, "isr_ea_march")
    return image, wts


def ea_march_host(densities, features, threshold: float = -1.0):
    """isr_ea_march_host: the same march as host code, NumPy (N,P), (N,P,F) -> (image (N,F+1), weights (N,P)).  For tests."""
    r, f = np.ascontiguousarray(densities, np.float32), np.ascontiguousarray(features, np.float32)
    if r.ndim != 2 or f.ndim != 3 or f.shape[:2] != r.shape:
        raise ValueError(f"ea_march_host: densities {r.shape}, features {f.shape}")
    N, P, F = f.shape
    image, wts = np.empty((N, F + 1), np.float32), np.empty((N, P), np.float32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_ea_march_host(hp(r), hp(f), N, P, F, float(threshold), hp(image), hp(wts)), "isr_ea_march_host")
    return image, wts


# ---- the backward of ea_march (include/isr_ea_grad.h)
def ea_grad_geometry() -> dict:
    """isr_ea_grad_geometry: the threads of a workgroup, the most rays one workgroup owns and the floats of LDS per array."""
    L = lib()
    return {"threads": L.isr_ea_grad_geometry(0), "max_group_rays": L.isr_ea_grad_geometry(1),
            "row_floats": L.isr_ea_grad_geometry(2)}


def ea_grad_rays_per_group(P: int) -> int:
    """isr_ea_grad_rays_per_group: the rays one workgroup of ea_march_backward owns at P samples per ray."""
    r = lib().isr_ea_grad_rays_per_group(int(P))
    if r < 1:
        raise ValueError(f"ea_grad_rays_per_group: P = {P} (1..4096)")
    return r


def _ea_grad_shapes(name: str, densities, features, dimage, dweights, threshold, need) -> tuple[int, int, int, float]:
    if densities.ndim != 2 or features.ndim != 3 or tuple(features.shape[:2]) != tuple(densities.shape):
        raise ValueError(f"{name}: densities {tuple(densities.shape)} and features {tuple(features.shape)} must be (N,P) and (N,P,F)")
    N, P, F = (int(v) for v in features.shape)
    if P < 1 or F < 1:
        raise ValueError(f"{name}: P < 1 or F < 1")
    if tuple(dimage.shape) != (N, F + 1):
        raise ValueError(f"{name}: dimage must be ({N},{F + 1}), got {tuple(dimage.shape)}")
    if dweights is not None and tuple(dweights.shape) != (N, P):
        raise ValueError(f"{name}: dweights must be ({N},{P}), got {tuple(dweights.shape)}")
    thr = float(threshold)
    if thr != thr:
        raise ValueError(f"{name}: threshold is NaN")
    if not (need[0] or need[1]):
        raise ValueError(f"{name}: neither gradient is asked for")
    return N, P, F, thr


def ea_march_backward(densities: torch.Tensor, features: torch.Tensor, dimage: torch.Tensor, dweights: torch.Tensor | None = None,
                      threshold: float = -1.0, need=(True, True)):
    """isr_ea_march_backward: the gradient of ea_march.  densities (N,P), features (N,P,F), dimage (N,F+1) [features |
    opacity] and dweights (N,P) or None (zeros), contiguous f32 on the device -> (ddensities (N,P), dfeatures (N,P,F)), None
    where need[i] is false: an adjoint recurrence per ray with no division and no float atomics, a function of the
    arguments only (include/isr_ea_grad.h).  In threshold mode ddensities is +0.  Nothing synchronises."""
    dev = require_cuda(densities, features, dimage, dweights)
    for t in (densities, features, dimage, dweights):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("ea_march_backward: every tensor must be contiguous float32")
    N, P, F, thr = _ea_grad_shapes("ea_march_backward", densities, features, dimage, dweights, threshold, need)
    dd = torch.empty((N, P), dtype=torch.float32, device=dev) if need[0] else None
    df = torch.empty((N, P, F), dtype=torch.float32, device=dev) if need[1] else None
    with torch.cuda.device(dev), _timed("ea_march_backward", 4.0 * N * P * F):
        rc = lib().isr_ea_march_backward(ptr(densities), ptr(features), N, P, F, thr, ptr(dimage), ptr(dweights), ptr(dd), ptr(df),
                                         current_stream(dev))
    check(rc, "isr_ea_march_backward")
    return dd, df


def ea_march_backward_host(densities, features, dimage, dweights=None, threshold: float = -1.0, need=(True, True)):
    """isr_ea_march_backward_host: the same gradient as host code over NumPy arrays.  For tests."""
    r, f, g = (np.ascontiguousarray(a, np.float32) for a in (densities, features, dimage))
    w = None if dweights is None else np.ascontiguousarray(dweights, np.float32)
    N, P, F, thr = _ea_grad_shapes("ea_march_backward_host", r, f, g, w, threshold, need)
    dd = np.empty((N, P), np.float32) if need[0] else None
    df = np.empty((N, P, F), np.float32) if need[1] else None
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_ea_march_backward_host(hp(r), hp(f), N, P, F, thr, hp(g), hp(w), hp(dd), hp(df)), "isr_ea_march_backward_host")
    return dd, df


def _host_i32(v, B: int, what: str):
    """A HOST (B,) int32 array for the C ABI (None stays None)."""
    if v is None:
        return None
    a = np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v).astype(np.int64).reshape(-1)
    if a.size != B:
        raise ValueError(f"fps_sample: {what} has {a.size} entries for {B} clouds")
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError(f"fps_sample: {what} does not fit int32")
    return np.ascontiguousarray(a, np.int32)


def fps_sample(points: torch.Tensor, K: int, lengths=None, start=None, want_radius: bool = False):
    """isr_fps_sample: farthest-point sampling of points (B,M,3) or (M,3) f32 -> idx (B,K) or (K,) int32, and with
    want_radius (idx, radius2) with radius2 f32 of the same shape (csrc/fps.hpp states the rule; rows k >= length hold -1 / 0).
    lengths, start: HOST integers per cloud (array-like, or a tensor that is copied to the host), None = all M / 0.
    K - 1 dependent steps, one launch each, on the current stream; nothing synchronises."""
    dev = require_cuda(points)
    single = points.ndim == 2
    pts = _f32c(points.unsqueeze(0) if single else points)
    if pts.ndim != 3 or pts.shape[2] != 3:
        raise ValueError(f"fps_sample: points must be (B,M,3) or (M,3), got {tuple(points.shape)}")
    B, M, K = pts.shape[0], pts.shape[1], int(K)
    lens, st = _host_i32(lengths, B, "lengths"), _host_i32(start, B, "start")
    L = lib()
    idx = torch.empty((B, max(K, 0)), dtype=torch.int32, device=dev)
    rad = torch.empty((B, max(K, 0)), dtype=torch.float32, device=dev) if want_radius else None
    nbytes = L.isr_fps_workspace_bytes(B, M)
    ws = workspace(dev, nbytes, "fps")
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    with torch.cuda.device(dev), _timed("fps_sample", float(B) * M * max(K - 1, 0)):
        rc = L.isr_fps_sample(ptr(pts), B, M, hp(lens), hp(st), K, ptr(idx), ptr(rad), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_fps_sample")
    if single:
        idx, rad = idx[0], (None if rad is None else rad[0])
    return (idx, rad) if want_radius else idx


def fps_sample_host(points, K: int, lengths=None, start=None):
    """isr_fps_sample_host: the same sampling as host code, NumPy (B,M,3) or (M,3) -> (idx int32, radius2 f32).  For tests."""
    p = np.ascontiguousarray(points, np.float32)
    single = p.ndim == 2
    p = p[None] if single else p
    if p.ndim != 3 or p.shape[2] != 3:
        raise ValueError(f"fps_sample_host: points must be (B,M,3) or (M,3), got {p.shape}")
    B, M, K = p.shape[0], p.shape[1], int(K)
    lens, st = _host_i32(lengths, B, "lengths"), _host_i32(start, B, "start")
    idx = np.empty((B, max(K, 0)), np.int32)
    rad = np.empty((B, max(K, 0)), np.float32)
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_fps_sample_host(hp(p), B, M, hp(lens), hp(st), K, hp(idx), hp(rad)), "isr_fps_sample_host")
    return (idx[0], rad[0]) if single else (idx, rad)


def marching_cubes(vol: torch.Tensor, iso: float, check_finite: bool = True):
    """isr_mc_count + isr_mc_emit: the iso-surface of vol (nx,ny,nz) f32 on the device at level iso (rounded to f32) -> (verts (V,3) f64 in
    INDEX space, tris (F,3) int32), on the device; an empty surface gives (0,3) arrays.  The rule (csrc/mc_extract.hpp, the
    table by tools/gen_mc_table.py) is the package's own: a corner is below when v < iso, the vertex of a crossing edge sits
    at (iso - va) / (vb - va) in f64, vertices in the order of the owning grid point then axis, triangles in cell order,
    right-hand normals pointing to the below side; a function of (vol, iso) only.  The totals are read between the two calls:
    the one synchronise.  check_finite (one more) refuses non-finite values, which a meaningful surface takes as a
    precondition."""
    dev = require_cuda(vol)
    v = _f32c(vol)
    if v.ndim != 3 or min(v.shape) < 2 or max(v.shape) > 1024 or v.numel() > 2 ** 28:
        raise ValueError(f"marching_cubes: vol must be (nx,ny,nz), every dimension 2..1024, at most 2^28 points, got "
                         f"{tuple(vol.shape)}")
    iso = float(iso)
    if iso != iso:
        raise ValueError("marching_cubes: iso is NaN")
    if check_finite and not bool(torch.isfinite(v).all()):
        raise ValueError("marching_cubes: non-finite values in vol (finite values are a precondition)")
    nx, ny, nz = v.shape
    L = lib()
    ws = workspace(dev, L.isr_mc_workspace_bytes(nx, ny, nz), "mc")
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        with _timed("mc_count", float(v.numel())):
            rc = L.isr_mc_count(ptr(v), nx, ny, nz, iso, ptr(counts), ptr(ws), ws.numel(), current_stream(dev))
        check(rc, "isr_mc_count")
        V, F = (int(c) for c in counts.cpu())
        verts = torch.empty((V, 3), dtype=torch.float64, device=dev)
        tris = torch.empty((F, 3), dtype=torch.int32, device=dev)
        if V or F:
            with _timed("mc_emit", float(v.numel())):
                rc = L.isr_mc_emit(ptr(v), nx, ny, nz, iso, ptr(ws), ws.numel(), ptr(verts) if V else None, V,
                                   ptr(tris) if F else None, F, current_stream(dev))
            check(rc, "isr_mc_emit")
    return verts, tris


def marching_cubes_host(vol, iso: float, check_finite: bool = True):
    """isr_mc_count_host + isr_mc_emit_host: the same extraction as host code, NumPy (nx,ny,nz) -> (verts (V,3) f64,
    tris (F,3) int32).  For tests."""
    v = np.ascontiguousarray(vol, np.float32)
    if v.ndim != 3:
        raise ValueError(f"marching_cubes_host: vol must be (nx,ny,nz), got {v.shape}")
    if check_finite and not np.isfinite(v).all():
        raise ValueError("marching_cubes_host: non-finite values in vol (finite values are a precondition)")
    nx, ny, nz = v.shape
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    counts = np.empty(2, np.int32)
    check(lib().isr_mc_count_host(hp(v), nx, ny, nz, float(iso), hp(counts)), "isr_mc_count_host")
    V, F = int(counts[0]), int(counts[1])
    verts, tris = np.empty((V, 3), np.float64), np.empty((F, 3), np.int32)
    check(lib().isr_mc_emit_host(hp(v), nx, ny, nz, float(iso), hp(verts) if V else None, V, hp(tris) if F else None, F),
          "isr_mc_emit_host")
    return verts, tris


def _cloud_n3(name: str, points, radius, check_finite: bool) -> float:
    if points.ndim != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"{name}: points must be (N,3) with N >= 1, got {tuple(points.shape)}")
    r = float(radius)
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"{name}: radius = {radius} must be finite and positive")
    if check_finite and not bool(torch.isfinite(points).all() if isinstance(points, torch.Tensor) else np.isfinite(points).all()):
        raise ValueError(f"{name}: non-finite coordinates (finite points are a precondition)")
    return r


def radius_count(points: torch.Tensor, radius: float, cap: int = 0, check_finite: bool = True) -> torch.Tensor:
    """isr_radius_count: points (N,3) f32 on the device -> counts (N,) int32, counts[i] the number of points j, i itself
    included, with d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) <= r * r in f32 (r the radius rounded to f32), clamped to cap
    when cap > 0.  A cell grid and a counting sort on the device (csrc/radius_count.hpp states the rule); exact, a function of
    (points, radius, cap) only.  Nothing synchronises but check_finite, which refuses non-finite coordinates (a precondition)."""
    dev = require_cuda(points)
    pts = _f32c(points)
    r = _cloud_n3("radius_count", pts, radius, check_finite)
    N = pts.shape[0]
    L = lib()
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    ws = workspace(dev, L.isr_radius_workspace_bytes(N), "radius")
    with torch.cuda.device(dev), _timed("radius_count", float(N)):
        rc = L.isr_radius_count(ptr(pts), N, r, int(cap), ptr(counts), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_radius_count")
    return counts


def radius_count_host(points, radius: float, cap: int = 0, check_finite: bool = True):
    """isr_radius_count_host: the same count as host code, NumPy (N,3) -> (N,) int32.  For tests."""
    p = np.ascontiguousarray(points, np.float32)
    r = _cloud_n3("radius_count_host", p, radius, check_finite)
    counts = np.empty(p.shape[0], np.int32)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_radius_count_host(hp(p), p.shape[0], r, int(cap), hp(counts)), "isr_radius_count_host")
    return counts


def radius_outlier_mask(points: torch.Tensor, nb_points: int, radius: float) -> torch.Tensor:
    """True where a point has more than nb_points points within `radius`, itself included:
    radius_count(points, radius, cap=nb_points + 1) > nb_points.  This is Open3D's RemoveRadiusOutliers
    (generateCors.py:257) AS FAR AS IT IS KNOWN FROM MEMORY — it keeps a point whose radius search, which finds the point
    itself, returns more than nb_points — Open3D is not available to compare against: the rule is unpinned."""
    return radius_count(points, radius, cap=int(nb_points) + 1) > int(nb_points)


def _knn_args(name: str, query, target, K, check_finite: bool) -> int:
    for what, a in (("query", query), ("target", target)):
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
            raise ValueError(f"{name}: {what} must be (N,3) with N >= 1, got {tuple(a.shape)}")
    K = int(K)
    if not 1 <= K <= min(target.shape[0], 1024):
        raise ValueError(f"{name}: K = {K} outside 1..min(Nt = {target.shape[0]}, 1024)")
    if check_finite:
        fin = (lambda a: bool(torch.isfinite(a).all())) if isinstance(query, torch.Tensor) else (lambda a: bool(np.isfinite(a).all()))
        if not (fin(query) and fin(target)):
            raise ValueError(f"{name}: non-finite coordinates (finite points are a precondition)")
    return K


def knn(query: torch.Tensor, target: torch.Tensor, K: int, want_d2: bool = True, check_finite: bool = True):
    """isr_knn: query (Nq,3), target (Nt,3) f32 on the device -> (idx (Nq,K) int32, d2 (Nq,K) f32 or None): per query the K
    targets smallest under (d2, index), ascending, d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in f32; among equal distances the
    lowest index first (csrc/knn.hpp states the rule).  Brute force over LDS tiles, a radix select per query; exact, a
    function of (query, target, K) only.  Nothing synchronises but check_finite, which refuses non-finite coordinates."""
    dev = require_cuda(query, target)
    q, t = _f32c(query), _f32c(target)
    K = _knn_args("knn", q, t, K, check_finite)
    Nq, Nt = q.shape[0], t.shape[0]
    L = lib()
    idx = torch.empty((Nq, K), dtype=torch.int32, device=dev)
    d2 = torch.empty((Nq, K), dtype=torch.float32, device=dev) if want_d2 else None
    ws = workspace(dev, L.isr_knn_workspace_bytes(Nq, Nt, K), "knn")
    with torch.cuda.device(dev), _timed("knn", float(Nq) * Nt):
        rc = L.isr_knn(ptr(q), Nq, ptr(t), Nt, K, ptr(idx), ptr(d2), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_knn")
    return idx, d2


def knn_host(query, target, K: int, want_d2: bool = True, check_finite: bool = True):
    """isr_knn_host: the same search as host code, NumPy (Nq,3), (Nt,3) -> (idx int32, d2 f32 or None).  For tests."""
    q, t = np.ascontiguousarray(query, np.float32), np.ascontiguousarray(target, np.float32)
    K = _knn_args("knn_host", q, t, K, check_finite)
    idx = np.empty((q.shape[0], K), np.int32)
    d2 = np.empty((q.shape[0], K), np.float32) if want_d2 else None
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_knn_host(hp(q), q.shape[0], hp(t), t.shape[0], K, hp(idx), hp(d2)), "isr_knn_host")
    return idx, d2


def _frames_args(name: str, points, idx) -> tuple[int, int]:
    if points.ndim != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"{name}: points must be (N,3) with N >= 1, got {tuple(points.shape)}")
    if idx.ndim != 2 or idx.shape[0] != points.shape[0] or not 1 <= idx.shape[1] <= 1024:
        raise ValueError(f"{name}: idx must be (N,K) with N = {points.shape[0]} and K in 1..1024, got {tuple(idx.shape)}")
    return points.shape[0], idx.shape[1]


def local_frames(points: torch.Tensor, idx: torch.Tensor, disambiguate: bool = True):
    """isr_local_frames: points (N,3) f32 and idx (N,K) (knn(points, points, K)[0]) on the device -> (curvatures (N,3) f64
    ascending, frames (N,3,3) f64, columns = eigenvectors, column 0 the normal): the eigen-decomposition of each
    neighbourhood's covariance about its own mean in f64 by cyclic Jacobi, and with disambiguate the sign rule
    include/isr_knn.h states (pytorch3d's as far as it is known: unpinned).  Nothing synchronises."""
    dev = require_cuda(points, idx)
    pts, ix = _f32c(points), idx.to(torch.int32).contiguous()
    N, K = _frames_args("local_frames", pts, ix)
    curv = torch.empty((N, 3), dtype=torch.float64, device=dev)
    frames = torch.empty((N, 3, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev), _timed("local_frames", float(N) * K):
        rc = lib().isr_local_frames(ptr(pts), N, ptr(ix), K, int(bool(disambiguate)), ptr(curv), ptr(frames), current_stream(dev))
    check(rc, "isr_local_frames")
    return curv, frames


def local_frames_host(points, idx, disambiguate: bool = True):
    """isr_local_frames_host: the same frames as host code, NumPy (N,3), (N,K) -> (curvatures, frames) f64.  For tests."""
    p, ix = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(idx, np.int32)
    N, K = _frames_args("local_frames_host", p, ix)
    curv, frames = np.empty((N, 3), np.float64), np.empty((N, 3, 3), np.float64)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(lib().isr_local_frames_host(hp(p), N, hp(ix), K, int(bool(disambiguate)), hp(curv), hp(frames)), "isr_local_frames_host")
    return curv, frames


RAYS_GRID, RAYS_MC = 0, 1       # ISR_RAYS_GRID / ISR_RAYS_MC of include/isr_rays.h


@dataclass(frozen=True)
class RaySpec:
    """Which rays a call of the isr_rays_* entries makes (include/isr_rays.h states the rules): host values only.
    mode RAYS_GRID: W x H rays per camera in raster order; mode RAYS_MC: n rays per camera from Philox under `seed`."""
    mode: int
    P: int
    min_depth: float
    max_depth: float
    W: int = 0
    H: int = 0
    n: int = 0
    min_x: float = -1.0
    max_x: float = 1.0
    min_y: float = -1.0
    max_y: float = 1.0
    stratified: bool = False
    seed: int = 0

    @property
    def rays_per_camera(self) -> int:
        return self.W * self.H if self.mode == RAYS_GRID else self.n


def _rays_check(name: str, spec: RaySpec, R, T, intr, camera_ids) -> int:
    """Shapes of the camera arrays and the limits of include/isr_rays.h; -> B."""
    if R.ndim != 3 or tuple(R.shape[1:]) != (3, 3) or R.shape[0] < 1:
        raise ValueError(f"{name}: R must be (B,3,3) with B >= 1, got {tuple(R.shape)}")
    B = R.shape[0]
    if tuple(T.shape) != (B, 3) or tuple(intr.shape) != (B, 4):
        raise ValueError(f"{name}: T must be ({B},3) and intr ({B},4), got {tuple(T.shape)} and {tuple(intr.shape)}")
    if camera_ids is not None and tuple(camera_ids.shape) != (B,):
        raise ValueError(f"{name}: camera_ids must be ({B},), got {tuple(camera_ids.shape)}")
    if spec.mode not in (RAYS_GRID, RAYS_MC):
        raise ValueError(f"{name}: mode = {spec.mode}")
    if spec.mode == RAYS_GRID and (spec.W < 1 or spec.H < 1):
        raise ValueError(f"{name}: grid {spec.W} x {spec.H} (each at least 1)")
    if spec.mode == RAYS_MC and spec.n < 1:
        raise ValueError(f"{name}: n = {spec.n} rays per camera (at least 1)")
    if B * spec.rays_per_camera > 2 ** 28:
        raise ValueError(f"{name}: {B} cameras x {spec.rays_per_camera} rays is more than 2^28")
    if not 1 <= spec.P <= 4096:
        raise ValueError(f"{name}: P = {spec.P} outside 1..4096")
    vals = (spec.min_x, spec.max_x, spec.min_y, spec.max_y, spec.min_depth, spec.max_depth)
    if not all(np.isfinite(v) for v in vals) or spec.min_x > spec.max_x or spec.min_y > spec.max_y:
        raise ValueError(f"{name}: ranges and depths must be finite with min <= max, got {vals}")
    if not 0 <= int(spec.seed) < 2 ** 64:
        raise ValueError(f"{name}: seed = {spec.seed} outside 0..2^64-1")
    return B


def _rays_args(spec: RaySpec, B: int, R, T, intr, camera_ids, p):
    return (spec.mode, p(R), p(T), p(intr), p(camera_ids), B, spec.W, spec.H, spec.n, spec.P, spec.min_x, spec.max_x, spec.min_y,
            spec.max_y, spec.min_depth, spec.max_depth, int(bool(spec.stratified)), int(spec.seed))


def _rays_mask(name: str, mask, B: int):
    if mask.ndim == 4 and mask.shape[-1] == 1:
        mask = mask[..., 0]
    if mask.ndim != 3 or mask.shape[0] != B or min(mask.shape[1:]) < 1:
        raise ValueError(f"{name}: mask must be ({B},mh,mw) or ({B},mh,mw,1), got {tuple(mask.shape)}")
    return mask


def _i32c(t):
    return None if t is None else t.to(torch.int32).contiguous()


def rays_bundle(spec: RaySpec, R: torch.Tensor, T: torch.Tensor, intr: torch.Tensor, camera_ids: torch.Tensor | None = None):
    """isr_rays_bundle: cameras R (B,3,3), T (B,3), intr (B,4) = (fx, fy, px, py) in NDC, f32 on the device -> every ray of
    `spec`: (origins (B,n,3), directions (B,n,3), lengths (B,n,P), xys (B,n,2)) f32 on the device.  Nothing synchronises."""
    dev = require_cuda(R, T, intr, camera_ids)
    R, T, intr, ids = _f32c(R), _f32c(T), _f32c(intr), _i32c(camera_ids)
    B = _rays_check("rays_bundle", spec, R, T, intr, ids)
    n = spec.rays_per_camera
    o = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    d = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    ln = torch.empty((B, n, spec.P), dtype=torch.float32, device=dev)
    xy = torch.empty((B, n, 2), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("rays_bundle", float(B) * n * spec.P):
        rc = lib().isr_rays_bundle(*_rays_args(spec, B, R, T, intr, ids, ptr), ptr(o), ptr(d), ptr(ln), ptr(xy), current_stream(dev))
    check(rc, "isr_rays_bundle")
    return o, d, ln, xy


def rays_select(spec: RaySpec, R: torch.Tensor, T: torch.Tensor, intr: torch.Tensor, mask: torch.Tensor,
                camera_ids: torch.Tensor | None = None, cap: int | None = None):
    """isr_rays_select_count + isr_rays_select_emit: the rays of `spec` whose xy falls on a non-zero pixel of mask (B,mh,mw[,1])
    (nutil.sample_images_at_mc_locs' nearest pixel; NaN counts), compacted in (camera, ray) order ->
    (origins (M,3), directions (M,3), lengths (M,P), xys (M,2), src (M,) int32: b * n + r of each kept ray, count (1,) int32),
    all on the device.  cap None: M = the count, read between the two calls — the one synchronise.  cap given: M = cap,
    nothing synchronises, rows from the count on are zeros and rows past cap are lost."""
    dev = require_cuda(R, T, intr, mask, camera_ids)
    R, T, intr, ids = _f32c(R), _f32c(T), _f32c(intr), _i32c(camera_ids)
    B = _rays_check("rays_select", spec, R, T, intr, ids)
    m = _f32c(_rays_mask("rays_select", mask, B))
    mh, mw = m.shape[1:]
    if cap is not None and not 0 <= int(cap) <= 2 ** 28:
        raise ValueError(f"rays_select: cap = {cap} outside 0..2^28")
    L = lib()
    args = _rays_args(spec, B, R, T, intr, ids, ptr)
    ws = workspace(dev, L.isr_rays_workspace_bytes(B, spec.rays_per_camera), "rays")
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        with _timed("rays_select_count", float(B) * spec.rays_per_camera):
            rc = L.isr_rays_select_count(*args, ptr(m), mh, mw, ptr(count), ptr(ws), ws.numel(), current_stream(dev))
        check(rc, "isr_rays_select_count")
        M = int(count.cpu()[0]) if cap is None else int(cap)
        o = torch.empty((M, 3), dtype=torch.float32, device=dev)
        d = torch.empty((M, 3), dtype=torch.float32, device=dev)
        ln = torch.empty((M, spec.P), dtype=torch.float32, device=dev)
        xy = torch.empty((M, 2), dtype=torch.float32, device=dev)
        src = torch.empty((M,), dtype=torch.int32, device=dev)
        if M:
            with _timed("rays_select_emit", float(M) * spec.P):
                rc = L.isr_rays_select_emit(*args, ptr(m), mh, mw, ptr(ws), ws.numel(), M, ptr(o), ptr(d), ptr(ln), ptr(xy), ptr(src),
                                            current_stream(dev))
            check(rc, "isr_rays_select_emit")
    return o, d, ln, xy, src, count


def _rays_host_arrays(R, T, intr, camera_ids):
    c = lambda a: np.ascontiguousarray(a, np.float32)
    return c(R), c(T), c(intr), None if camera_ids is None else np.ascontiguousarray(camera_ids, np.int32)


def _hp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def rays_bundle_host(spec: RaySpec, R, T, intr, camera_ids=None):
    """isr_rays_bundle_host: the same bundle as host code over NumPy arrays.  For tests."""
    R, T, intr, ids = _rays_host_arrays(R, T, intr, camera_ids)
    B = _rays_check("rays_bundle_host", spec, R, T, intr, ids)
    n = spec.rays_per_camera
    o, d = np.empty((B, n, 3), np.float32), np.empty((B, n, 3), np.float32)
    ln, xy = np.empty((B, n, spec.P), np.float32), np.empty((B, n, 2), np.float32)
    check(lib().isr_rays_bundle_host(*_rays_args(spec, B, R, T, intr, ids, _hp), _hp(o), _hp(d), _hp(ln), _hp(xy)),
          "isr_rays_bundle_host")
    return o, d, ln, xy


def rays_select_host(spec: RaySpec, R, T, intr, mask, camera_ids=None, cap: int | None = None):
    """isr_rays_select_count_host + isr_rays_select_emit_host: rays_select as host code over NumPy arrays; count an int."""
    R, T, intr, ids = _rays_host_arrays(R, T, intr, camera_ids)
    B = _rays_check("rays_select_host", spec, R, T, intr, ids)
    m = np.ascontiguousarray(_rays_mask("rays_select_host", np.asarray(mask), B), np.float32)
    mh, mw = m.shape[1:]
    args = _rays_args(spec, B, R, T, intr, ids, _hp)
    cnt = np.empty(1, np.int32)
    check(lib().isr_rays_select_count_host(*args, _hp(m), mh, mw, _hp(cnt)), "isr_rays_select_count_host")
    M = int(cnt[0]) if cap is None else int(cap)
    o, d = np.empty((M, 3), np.float32), np.empty((M, 3), np.float32)
    ln, xy, src = np.empty((M, spec.P), np.float32), np.empty((M, 2), np.float32), np.empty((M,), np.int32)
    if M:
        check(lib().isr_rays_select_emit_host(*args, _hp(m), mh, mw, M, _hp(o), _hp(d), _hp(ln), _hp(xy), _hp(src)),
              "isr_rays_select_emit_host")
    return o, d, ln, xy, src, int(cnt[0])


def _sample_shapes(name: str, images, xys) -> tuple[int, int, int, int, int]:
    if images.ndim != 4 or min(images.shape) < 1 or images.shape[3] > 4096:
        raise ValueError(f"{name}: images must be (B,H,W,C), every side at least 1 and C at most 4096, got {tuple(images.shape)}")
    B, H, W, C = images.shape
    if xys.ndim < 3 or xys.shape[0] != B or xys.shape[-1] != 2 or 0 in tuple(xys.shape):
        raise ValueError(f"{name}: xys must be ({B},...,2) and not empty, got {tuple(xys.shape)}")
    n = int(np.prod(xys.shape[1:-1]))
    if B * n > 2 ** 28 or B * n * C >= 2 ** 31:
        raise ValueError(f"{name}: {B} x {n} locations x {C} channels is too many (B n <= 2^28, B n C < 2^31)")
    return B, H, W, C, n


def sample_at_rays(images: torch.Tensor, xys: torch.Tensor) -> torch.Tensor:
    """isr_sample_nearest: images (B,H,W,C) sampled at the NDC locations xys (B,...,2) -> (B,...,C) f32, on the device:
    grid_sample(images.permute(0,3,1,2), -xys, align_corners=True, mode='nearest') with zero padding (nutil.py:188-193),
    value for value.  Nothing synchronises.  Not differentiable: the result carries no grad_fn; the route with a gradient
    is rays.sample_images_at_mc_locs, whose backward is sample_at_rays_backward."""
    dev = require_cuda(images, xys)
    im, xy = _f32c(images), _f32c(xys)
    B, H, W, C, n = _sample_shapes("sample_at_rays", im, xy)
    out = torch.empty((*xy.shape[:-1], C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("sample_nearest", float(B) * n * C):
        rc = lib().isr_sample_nearest(ptr(im), B, H, W, C, ptr(xy), n, ptr(out), current_stream(dev))
    check(rc, "isr_sample_nearest")
    return out


def sample_at_rays_host(images, xys):
    """isr_sample_nearest_host: the same sampling as host code over NumPy arrays.  For tests."""
    im, xy = np.ascontiguousarray(images, np.float32), np.ascontiguousarray(xys, np.float32)
    B, H, W, C, n = _sample_shapes("sample_at_rays_host", im, xy)
    out = np.empty((*xy.shape[:-1], C), np.float32)
    check(lib().isr_sample_nearest_host(_hp(im), B, H, W, C, _hp(xy), n, _hp(out)), "isr_sample_nearest_host")
    return out


# ---- the backward of sample_at_rays (include/isr_sample_grad.h)
def sample_grad_geometry() -> dict:
    """isr_sample_grad_geometry: the largest n sorted in LDS, the radix sort's keys per block and the bits of its digit."""
    L = lib()
    return {"lds_rays": L.isr_sample_grad_geometry(0), "block_keys": L.isr_sample_grad_geometry(1),
            "digit_bits": L.isr_sample_grad_geometry(2)}


def _sample_grad_shapes(name: str, dout, xys, H: int, W: int) -> tuple[int, int, int]:
    if xys.ndim < 3 or xys.shape[-1] != 2 or 0 in tuple(xys.shape):
        raise ValueError(f"{name}: xys must be (B,...,2) and not empty, got {tuple(xys.shape)}")
    if dout.ndim != xys.ndim or tuple(dout.shape[:-1]) != tuple(xys.shape[:-1]) or not 1 <= dout.shape[-1] <= 4096:
        raise ValueError(f"{name}: dout must be {tuple(xys.shape[:-1])} + (C,) with C in 1..4096, got {tuple(dout.shape)}")
    B, C = int(xys.shape[0]), int(dout.shape[-1])
    n = int(np.prod(xys.shape[1:-1]))
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W >= 2 ** 31 - 1 or B * H * W * C >= 2 ** 40:
        raise ValueError(f"{name}: an image of {H} x {W} pixels, {B} of them with {C} channels (H W < 2^31 - 1, B H W C < 2^40)")
    if B * n > 2 ** 28 or B * n * C >= 2 ** 31:
        raise ValueError(f"{name}: {B} x {n} locations x {C} channels is too many (B n <= 2^28, B n C < 2^31)")
    return B, C, n


def sample_at_rays_backward(dout: torch.Tensor, xys: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """isr_sample_nearest_backward: the gradient of sample_at_rays with respect to its images.  dout (B,...,C) at the NDC
    locations xys (B,...,2) -> dimages (B,H,W,C) f32 on the device: per (pixel, channel) the f32 sum of the pixel's rays in
    ray order from +0, a function of the arguments only (no float atomics).  Nothing synchronises."""
    dev = require_cuda(dout, xys)
    g, xy = _f32c(dout), _f32c(xys)
    B, C, n = _sample_grad_shapes("sample_at_rays_backward", g, xy, H, W)
    out = torch.empty((B, int(H), int(W), C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nbytes = lib().isr_sample_grad_workspace_bytes(B, int(H), int(W), n)
        if nbytes == 0:
            check(-1, "isr_sample_grad_workspace_bytes")
        ws = workspace(dev, nbytes, tag="sample_grad")
        with _timed("sample_nearest_backward", float(B) * n * C):
            rc = lib().isr_sample_nearest_backward(ptr(g), B, int(H), int(W), C, ptr(xy), n, ptr(out), ptr(ws), ws.numel(),
                                                   current_stream(dev))
    check(rc, "isr_sample_nearest_backward")
    return out


def sample_at_rays_backward_host(dout, xys, H: int, W: int):
    """isr_sample_nearest_backward_host: the same gradient as host code over NumPy arrays.  For tests."""
    g, xy = np.ascontiguousarray(dout, np.float32), np.ascontiguousarray(xys, np.float32)
    B, C, n = _sample_grad_shapes("sample_at_rays_backward_host", g, xy, H, W)
    out = np.empty((B, int(H), int(W), C), np.float32)
    check(lib().isr_sample_nearest_backward_host(_hp(g), B, int(H), int(W), C, _hp(xy), n, _hp(out)),
          "isr_sample_nearest_backward_host")
    return out


def philox_host(counter, key):
    """isr_rays_philox_host: Philox4x32-10 of counter (4 words) under key (2 words) -> (words (4,) uint32, units (4,) f32)."""
    c, k = np.ascontiguousarray(counter, np.uint32), np.ascontiguousarray(key, np.uint32)
    if c.shape != (4,) or k.shape != (2,):
        raise ValueError(f"philox_host: counter must be 4 words and key 2, got {c.shape} and {k.shape}")
    words, units = np.empty(4, np.uint32), np.empty(4, np.float32)
    check(lib().isr_rays_philox_host(_hp(c), _hp(k), _hp(words), _hp(units)), "isr_rays_philox_host")
    return words, units


def _resample_check(name: str, a, w, a_cols_minus_w: int, n_samples, eps, seed, ray_ids) -> tuple[int, int]:
    """Shapes and limits of include/isr_resample.h for rows a (N, w_cols + a_cols_minus_w) and w (N, w_cols); -> (N, w_cols)."""
    if a.ndim != 2 or w.ndim != 2 or a.shape[0] != w.shape[0] or a.shape[1] != w.shape[1] + a_cols_minus_w:
        raise ValueError(f"{name}: rows of {tuple(a.shape)} and {tuple(w.shape)} do not belong together "
                         f"(expected (N, {'P' if a_cols_minus_w == 0 else 'nb+1'}) and (N, {'P' if a_cols_minus_w == 0 else 'nb'}))")
    if a.dtype != w.dtype or str(a.dtype).split(".")[-1] != "float32":
        raise ValueError(f"{name}: float32 arrays only, got {a.dtype} and {w.dtype}")
    N, P = a.shape[0], w.shape[1] + 2 * a_cols_minus_w           # P: the lengths the bins came from
    if not 3 <= P <= 1024:
        raise ValueError(f"{name}: P = {P} outside 3..1024 (nb = P - 2)")
    if not 1 <= int(n_samples) <= 1024:
        raise ValueError(f"{name}: n_samples = {n_samples} outside 1..1024")
    if N > 2 ** 28:
        raise ValueError(f"{name}: {N} rays is more than 2^28")
    if not (float(eps) > 0.0 and np.isfinite(np.float32(eps)) and np.float32(eps) > 0):
        raise ValueError(f"{name}: eps = {eps} must be positive and finite in float32")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"{name}: seed = {seed} outside 0..2^64-1")
    if ray_ids is not None and tuple(ray_ids.shape) != (N,):
        raise ValueError(f"{name}: ray_ids must be ({N},), got {tuple(ray_ids.shape)}")
    return N, w.shape[1]


def _resample_device(name: str, a: torch.Tensor, w: torch.Tensor, ray_ids):
    dev = require_cuda(a, w, ray_ids)
    if not (a.is_contiguous() and w.is_contiguous()):
        raise ValueError(f"{name}: the arrays must be contiguous")
    return dev, _i32c(ray_ids)


def sample_pdf(bins: torch.Tensor, weights: torch.Tensor, n_samples: int, det: bool = False, eps: float = 1e-5, seed: int = 0,
               ray_ids: torch.Tensor | None = None) -> torch.Tensor:
    """isr_sample_pdf: bins (N, nb+1), weights (N, nb) contiguous f32 on the device -> samples (N, n_samples), unsorted, in
    sample order: pytorch3d's sample_pdf as include/isr_resample.h states it.  det: units linspace(0, 1, n), otherwise Philox
    under `seed` and ray_ids (N,) int32 (default 0 .. N-1).  One launch; nothing synchronises."""
    dev, ids = _resample_device("sample_pdf", bins, weights, ray_ids)
    N, nb = _resample_check("sample_pdf", bins, weights, 1, n_samples, eps, seed, ids)
    out = torch.empty((N, int(n_samples)), dtype=torch.float32, device=dev)
    if N:
        with torch.cuda.device(dev), _timed("sample_pdf", float(N) * (2 * nb + 1 + int(n_samples)) * 4):
            rc = lib().isr_sample_pdf(ptr(bins), ptr(weights), N, nb, int(n_samples), int(bool(det)), float(eps), int(seed), ptr(ids),
                                      ptr(out), current_stream(dev))
        check(rc, "isr_sample_pdf")
    return out


def resample_lengths(lengths: torch.Tensor, ray_weights: torch.Tensor, n_samples: int, add_input_samples: bool = True,
                     det: bool = False, eps: float = 1e-5, seed: int = 0, ray_ids: torch.Tensor | None = None) -> torch.Tensor:
    """isr_resample_lengths: lengths (N, P), ray_weights (N, P) contiguous f32 on the device -> the sorted depths of the fine
    pass (N, n_samples + P) (or (N, n_samples) without add_input_samples): ProbabilisticRaysampler.forward of pren.py:427-457
    as include/isr_resample.h states it.  One launch; nothing synchronises."""
    dev, ids = _resample_device("resample_lengths", lengths, ray_weights, ray_ids)
    N, P = _resample_check("resample_lengths", lengths, ray_weights, 0, n_samples, eps, seed, ids)
    P_out = int(n_samples) + (P if add_input_samples else 0)
    out = torch.empty((N, P_out), dtype=torch.float32, device=dev)
    if N:
        with torch.cuda.device(dev), _timed("resample_lengths", float(N) * (2 * P + P_out) * 4):
            rc = lib().isr_resample_lengths(ptr(lengths), ptr(ray_weights), N, P, int(n_samples), int(bool(add_input_samples)),
                                            int(bool(det)), float(eps), int(seed), ptr(ids), ptr(out), current_stream(dev))
        check(rc, "isr_resample_lengths")
    return out


def _resample_host(name: str, a, w, ray_ids):
    if getattr(a, "dtype", None) != np.float32 or getattr(w, "dtype", None) != np.float32:
        raise ValueError(f"{name}: float32 NumPy arrays only")
    ids = None if ray_ids is None else np.ascontiguousarray(ray_ids, np.int32)
    return np.ascontiguousarray(a), np.ascontiguousarray(w), ids


def sample_pdf_host(bins, weights, n_samples: int, det: bool = False, eps: float = 1e-5, seed: int = 0, ray_ids=None):
    """isr_sample_pdf_host: sample_pdf as host code over NumPy arrays.  For tests."""
    b, w, ids = _resample_host("sample_pdf_host", bins, weights, ray_ids)
    N, nb = _resample_check("sample_pdf_host", b, w, 1, n_samples, eps, seed, ids)
    out = np.empty((N, int(n_samples)), np.float32)
    check(lib().isr_sample_pdf_host(_hp(b), _hp(w), N, nb, int(n_samples), int(bool(det)), float(eps), int(seed), _hp(ids), _hp(out)),
          "isr_sample_pdf_host")
    return out


def resample_lengths_host(lengths, ray_weights, n_samples: int, add_input_samples: bool = True, det: bool = False,
                          eps: float = 1e-5, seed: int = 0, ray_ids=None):
    """isr_resample_lengths_host: resample_lengths as host code over NumPy arrays.  For tests."""
    ln, w, ids = _resample_host("resample_lengths_host", lengths, ray_weights, ray_ids)
    N, P = _resample_check("resample_lengths_host", ln, w, 0, n_samples, eps, seed, ids)
    out = np.empty((N, int(n_samples) + (P if add_input_samples else 0)), np.float32)
    check(lib().isr_resample_lengths_host(_hp(ln), _hp(w), N, P, int(n_samples), int(bool(add_input_samples)), int(bool(det)),
                                          float(eps), int(seed), _hp(ids), _hp(out)), "isr_resample_lengths_host")
    return out


def resample_rays_per_group(P: int, n_samples: int, add_input_samples: bool = True, sorted_rows: bool = True) -> int:
    """isr_resample_rays_per_group: the rays one workgroup of the resample kernel owns for this shape (tests and tools)."""
    R = lib().isr_resample_rays_per_group(int(P), int(n_samples), int(bool(add_input_samples)), int(bool(sorted_rows)))
    if R < 1:
        check(-1, "isr_resample_rays_per_group")
    return R


# ---- the contrastive key loss and its gradient (include/isr_contrastive.h)

def _contrastive_shape(name: str, q, k, n):
    """-> (B, S, M, D, Bn) of q (B, S, D), k (B, S, D), n (Bn, M, D); the library checks the limits."""
    if q.ndim != 3 or tuple(k.shape) != tuple(q.shape) or n.ndim != 3 or n.shape[2] != q.shape[2]:
        raise ValueError(f"{name}: q (B, S, D), k (B, S, D), n (Bn, M, D) expected, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(n.shape)}")
    return q.shape[0], q.shape[1], n.shape[1], q.shape[2], n.shape[0]


def _contrastive_device(name: str, *tensors):
    dev = require_cuda(*tensors)
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"{name}: contiguous float32 tensors only")
    return dev


def _contrastive_workspace(dev, shape) -> torch.Tensor:
    nbytes = lib().isr_contrastive_workspace_bytes(*shape)
    if nbytes == 0:
        check(-1, "isr_contrastive_workspace_bytes")
    return workspace(dev, nbytes, "contrastive")


def contrastive_forward(q: torch.Tensor, k: torch.Tensor, n: torch.Tensor, scale: float = 1e-3):
    """isr_contrastive_forward: q (B, S, D), k (B, S, D), n (Bn, M, D) contiguous f32 on the device, Bn in {1, B} ->
    (m, t, pos, rows) of shape (B, S) and loss (0-d): the cross-entropy of every query against its positive and its negative
    keys as include/isr_contrastive.h states it, scaled.  No (S, M) array is made; nothing synchronises."""
    dev = _contrastive_device("contrastive_forward", q, k, n)
    shape = _contrastive_shape("contrastive_forward", q, k, n)
    B, S, M, D, Bn = shape
    ws = _contrastive_workspace(dev, shape)
    m, t, pos, rows = (torch.empty((B, S), dtype=torch.float32, device=dev) for _ in range(4))
    loss = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("contrastive_forward", 2.0 * B * S * M * D * 2):
        rc = lib().isr_contrastive_forward(ptr(q), ptr(k), ptr(n), B, S, M, D, Bn, float(scale), ptr(m), ptr(t), ptr(pos), ptr(rows),
                                           ptr(loss), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_contrastive_forward")
    return m, t, pos, rows, loss


def contrastive_backward(q: torch.Tensor, k: torch.Tensor, n: torch.Tensor, m: torch.Tensor, t: torch.Tensor,
                         g: torch.Tensor | None = None, scale: float = 1e-3, need=(True, True, True)):
    """isr_contrastive_backward: the gradients (dq, dk, dn) of contrastive_forward's loss from its saved m and t; g: the
    upstream gradient as a device tensor of one f32 (read on the device; None for 1); need: which of the three to compute
    (the others are None).  Nothing synchronises."""
    dev = _contrastive_device("contrastive_backward", q, k, n, m, t, g)
    shape = _contrastive_shape("contrastive_backward", q, k, n)
    B, S, M, D, Bn = shape
    if m.numel() != B * S or t.numel() != B * S or (g is not None and g.numel() != 1):
        raise ValueError("contrastive_backward: m and t must hold B S values, g one")
    ws = _contrastive_workspace(dev, shape)
    dq = torch.empty_like(q) if need[0] else None
    dk = torch.empty_like(k) if need[1] else None
    dn = torch.empty_like(n) if need[2] else None
    with torch.cuda.device(dev), _timed("contrastive_backward", 2.0 * B * S * M * D * 4):
        rc = lib().isr_contrastive_backward(ptr(q), ptr(k), ptr(n), B, S, M, D, Bn, float(scale), ptr(m), ptr(t), ptr(g), ptr(dq),
                                            ptr(dk), ptr(dn), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_contrastive_backward")
    return dq, dk, dn


def _contrastive_host(name: str, *arrays):
    for a in arrays:
        if a is not None and getattr(a, "dtype", None) != np.float32:
            raise ValueError(f"{name}: float32 NumPy arrays only")
    return tuple(None if a is None else np.ascontiguousarray(a) for a in arrays)


def contrastive_forward_host(q, k, n, scale: float = 1e-3):
    """isr_contrastive_forward_host: contrastive_forward as host code over NumPy arrays.  For tests."""
    q, k, n = _contrastive_host("contrastive_forward_host", q, k, n)
    B, S, M, D, Bn = _contrastive_shape("contrastive_forward_host", q, k, n)
    m, t, pos, rows = (np.empty((B, S), np.float32) for _ in range(4))
    loss = np.empty((), np.float32)
    check(lib().isr_contrastive_forward_host(_hp(q), _hp(k), _hp(n), B, S, M, D, Bn, float(scale), _hp(m), _hp(t), _hp(pos), _hp(rows),
                                             _hp(loss)), "isr_contrastive_forward_host")
    return m, t, pos, rows, loss


def contrastive_backward_host(q, k, n, m, t, g=None, scale: float = 1e-3, need=(True, True, True)):
    """isr_contrastive_backward_host: contrastive_backward as host code over NumPy arrays.  For tests."""
    q, k, n, m, t = _contrastive_host("contrastive_backward_host", q, k, n, m, t)
    B, S, M, D, Bn = _contrastive_shape("contrastive_backward_host", q, k, n)
    if m.size != B * S or t.size != B * S:
        raise ValueError("contrastive_backward_host: m and t must hold B S values")
    gp = None if g is None else np.array([g], np.float32)
    dq = np.empty_like(q) if need[0] else None
    dk = np.empty_like(k) if need[1] else None
    dn = np.empty_like(n) if need[2] else None
    check(lib().isr_contrastive_backward_host(_hp(q), _hp(k), _hp(n), B, S, M, D, Bn, float(scale), _hp(m), _hp(t), _hp(gp), _hp(dq),
                                              _hp(dk), _hp(dn)), "isr_contrastive_backward_host")
    return dq, dk, dn


def contrastive_geometry() -> dict:
    """isr_contrastive_geometry: the widths of the contrastive kernels (tests and tools)."""
    return {name: lib().isr_contrastive_geometry(i) for i, name in enumerate(("group", "tile", "range_rows", "reduce"))}


def contrastive_column_splits(B: int, S: int, M: int, D: int, Bn: int) -> int:
    """isr_contrastive_column_splits: the 1024-row ranges the dn pass is split into for this shape (1: not split)."""
    r = lib().isr_contrastive_column_splits(int(B), int(S), int(M), int(D), int(Bn))
    if r < 1:
        check(-1, "isr_contrastive_column_splits")
    return r


# ---- the key field's backward and the device-side packing (include/isr_field_grad.h)

def field_grad_geometry() -> dict:
    """isr_field_grad_geometry: the widths of the backward (tests and tools): the chain length of a weight sum, the tile of
    points a workgroup takes, the largest slab of points whose activations the workspace holds at a time, and the batch of
    points whose block sums it holds."""
    return {name: lib().isr_field_grad_geometry(i) for i, name in enumerate(("chain", "tile", "slab", "batch"))}


def field_param_sizes(widths) -> tuple[int, int]:
    """-> (entries of every W, entries of every b) of a field of these widths, the lengths of the standard layout."""
    w = [int(v) for v in widths]
    return sum(a * b for a, b in zip(w[:-1], w[1:])), sum(w[1:])


def _field_header(widths, omegas):
    """-> (n_layers, widths pointer, its array, omega array, sine array) for the entries that take the field's shape."""
    nl = len(widths) - 1
    if len(omegas) != nl:
        raise ValueError(f"{nl} layers but {len(omegas)} omegas")
    w = (ctypes.c_int32 * len(widths))(*[int(v) for v in widths])
    om = (ctypes.c_float * nl)(*[0.0 if o is None else float(o) for o in omegas])
    sine = (ctypes.c_int32 * nl)(*[0 if o is None else 1 for o in omegas])
    return nl, ctypes.cast(w, ctypes.c_void_p), w, om, sine


def _flat_f32(name: str, what: str, t: torch.Tensor, numel: int) -> None:
    if t.dtype != torch.float32 or t.ndim != 1 or t.numel() != numel or not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous ({numel},) float32, got {tuple(t.shape)} {t.dtype}")


def field_pack_device(widths, W: torch.Tensor, b: torch.Tensor, omegas, pack: torch.Tensor | None = None,
                      packT: torch.Tensor | None = None):
    """isr_field_pack_device: W and b in the standard layout (every layer's (out, in) matrix row-major, layer after layer, flat;
    the biases likewise) on the device -> (pack, packT): the forward pack, byte for byte isr_field_pack's, and the transposed
    pack of the backward.  Every word of both is written (into `pack` / `packT` when given); nothing synchronises."""
    dev = require_cuda(W, b, pack, packT)
    nw, nb = field_param_sizes(widths)
    _flat_f32("field_pack_device", "W", W, nw)
    _flat_f32("field_pack_device", "b", b, nb)
    nl, wp, _keep, om, sine = _field_header(widths, omegas)
    L = lib()
    words, wordsT = L.isr_field_pack_bytes(nl, wp) // 4, L.isr_field_grad_pack_bytes(nl, wp) // 4
    if words == 0 or wordsT == 0:
        check(-1, "isr_field_pack_bytes")
    if pack is None:
        pack = torch.empty(words, dtype=torch.float32, device=dev)
    if packT is None:
        packT = torch.empty(wordsT, dtype=torch.float32, device=dev)
    _flat_f32("field_pack_device", "pack", pack, words)
    _flat_f32("field_pack_device", "packT", packT, wordsT)
    with torch.cuda.device(dev), _timed("field_pack_device", 0.0):
        rc = L.isr_field_pack_device(nl, wp, ptr(W), ptr(b), ctypes.cast(om, ctypes.c_void_p), ctypes.cast(sine, ctypes.c_void_p),
                                     ptr(pack), words * 4, ptr(packT), wordsT * 4, current_stream(dev))
    check(rc, "isr_field_pack_device")
    return pack, packT


def field_backward_flops(widths) -> float:
    """Multiply-adds x 2 of one point through the backward as issued: the forward again, the u pass (every layer but the
    first) and the dW pass."""
    w = [int(v) for v in widths]
    return 2.0 * field_flops(w) + 2.0 * sum(a * b for a, b in zip(w[1:-1], w[2:]))


def field_backward(pack: torch.Tensor, packT: torch.Tensor, widths, points: torch.Tensor, dout: torch.Tensor,
                   need=(True, True), slab: int | None = None):
    """isr_field_backward: points (N,3) f32 and the upstream gradient dout (N, ld) f32, ld >= widths[-1] (only columns below
    widths[-1] are read) -> (dW, db) flat in the standard layout (field_param_sizes), every entry written; need: which of the
    two to compute (the other is None).  The forward is recomputed from the points; pack and packT are field_pack_device's.
    slab: work through N this many points at a time (a multiple of the chain length; tests) instead of the default.  Nothing
    synchronises."""
    dev = require_cuda(pack, packT, points, dout)
    N, o = _points_n3("field_backward", points), int(widths[-1])
    if dout.dtype != torch.float32 or dout.ndim != 2 or dout.shape[0] != N or dout.shape[1] < o or not dout.is_contiguous():
        raise ValueError(f"field_backward: dout must be contiguous ({N}, >= {o}) float32, got {tuple(dout.shape)} {dout.dtype}")
    nw, nb = field_param_sizes(widths)
    pk, nbytes, nl, wp, _keep = _field_args(pack, widths, len(widths) - 1)
    L = lib()
    if slab is None:
        ws_bytes = L.isr_field_grad_workspace_bytes(nl, wp, N)
        ws = workspace(dev, ws_bytes, "field_grad") if ws_bytes else None
    else:
        chain = L.isr_field_grad_geometry(0)
        if slab < chain or slab % chain:
            raise ValueError(f"field_backward: slab {slab} is not a multiple of the chain length {chain}")
        ws_bytes = L.isr_field_grad_workspace_bytes(nl, wp, int(slab))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    if ws_bytes == 0:
        check(-1, "isr_field_grad_workspace_bytes")
    dW = torch.empty(nw, dtype=torch.float32, device=dev) if need[0] else None
    db = torch.empty(nb, dtype=torch.float32, device=dev) if need[1] else None
    with torch.cuda.device(dev), _timed("field_backward", N * field_backward_flops(widths)):
        rc = L.isr_field_backward(pk, nbytes, ptr(packT), packT.numel() * packT.element_size(), nl, wp, ptr(points) if N else None,
                                  N, ptr(dout) if N else None, dout.shape[1], ptr(dW), ptr(db), ptr(ws), ws_bytes,
                                  current_stream(dev))
    check(rc, "isr_field_backward")
    return dW, db


def field_backward_host(pack_host, widths, points, dout, need=(True, True)):
    """isr_field_backward_host: field_backward as host code over NumPy arrays (pack_host: isr_field_pack's words, e.g.
    KeyField.pack_host).  For tests."""
    pack_host = np.ascontiguousarray(pack_host, np.float32)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    dout = np.ascontiguousarray(dout, np.float32)
    if dout.ndim != 2 or dout.shape[0] != pts.shape[0]:
        raise ValueError(f"field_backward_host: dout {dout.shape} for {pts.shape[0]} points")
    nw, nb = field_param_sizes(widths)
    w = np.asarray(widths, np.int32)
    dW = np.empty(nw, np.float32) if need[0] else None
    db = np.empty(nb, np.float32) if need[1] else None
    check(lib().isr_field_backward_host(_hp(pack_host), pack_host.nbytes, len(w) - 1, _hp(w), _hp(pts), pts.shape[0], _hp(dout),
                                        dout.shape[1], _hp(dW), _hp(db)), "isr_field_backward_host")
    return dW, db


def field_cos_host(a):
    """isr_field_cos_host: cos32 of every element of a NumPy f32 array.  For tests."""
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    check(lib().isr_field_cos_host(_hp(a), a.size, _hp(out)), "isr_field_cos_host")
    return out


# ---- the radiance field's backward and the device-side packing (include/isr_radiance_grad.h)

def radiance_grad_geometry() -> dict:
    """isr_radiance_grad_geometry: the chain length of a weight sum, the tile of points a workgroup takes, the largest slab of
    points whose per-layer inputs the workspace holds at a time, and the batch of points whose block sums it holds."""
    return {name: lib().isr_radiance_grad_geometry(i) for i, name in enumerate(("chain", "tile", "slab", "batch"))}


def radiance_param_sizes(widths, H: int, Wc: int, C: int) -> tuple[int, int]:
    """-> (entries of every W, entries of every b) of isr_radiance_pack's layout: the hidden matrices, the density row,
    W1 (Wc, Wt + 6H), W2 (C, Wc); the biases likewise."""
    w = [6 * int(H)] + [int(v) for v in widths]
    Wt = w[-1]
    return (sum(a * b for a, b in zip(w[:-1], w[1:])) + Wt + int(Wc) * (Wt + 6 * int(H)) + int(C) * int(Wc),
            sum(w[1:]) + 1 + int(Wc) + int(C))


def radiance_param_shapes(widths, H: int, Wc: int, C: int) -> list[tuple[int, int]]:
    """The (out, in) of every matrix of that layout, in its order."""
    w = [6 * int(H)] + [int(v) for v in widths]
    return [(o, i) for i, o in zip(w[:-1], w[1:])] + [(1, w[-1]), (int(Wc), w[-1] + 6 * int(H)), (int(C), int(Wc))]


def _radiance_shape(widths, H, Wc, C):
    w = (ctypes.c_int32 * len(widths))(*[int(v) for v in widths])
    return (len(widths), ctypes.cast(w, ctypes.c_void_p), int(H), int(Wc), int(C)), w      # w: kept alive by the caller


def radiance_pack_device(widths, H: int, Wc: int, C: int, frequencies, beta: float, W: torch.Tensor, b: torch.Tensor,
                         pack: torch.Tensor | None = None, packT: torch.Tensor | None = None):
    """isr_radiance_pack_device: W and b flat in isr_radiance_pack's layout (radiance_param_sizes) on the device, the H
    frequencies on the host -> (pack, packT): the forward pack, byte for byte isr_radiance_pack's, and the transposed pack of
    the backward.  Every word of both is written (into `pack` / `packT` when given); nothing synchronises."""
    dev = require_cuda(W, b, pack, packT)
    nw, nb = radiance_param_sizes(widths, H, Wc, C)
    _flat_f32("radiance_pack_device", "W", W, nw)
    _flat_f32("radiance_pack_device", "b", b, nb)
    fr = np.ascontiguousarray(frequencies.detach().cpu().numpy() if isinstance(frequencies, torch.Tensor) else frequencies,
                              np.float32).reshape(-1)
    if fr.shape[0] != int(H):
        raise ValueError(f"radiance_pack_device: {fr.shape[0]} frequencies, H = {H}")
    shape, _keep = _radiance_shape(widths, H, Wc, C)
    L = lib()
    words, wordsT = L.isr_radiance_pack_bytes(*shape) // 4, L.isr_radiance_grad_pack_bytes(*shape) // 4
    if words == 0 or wordsT == 0:
        check(-1, "isr_radiance_pack_bytes")
    if pack is None:
        pack = torch.empty(words, dtype=torch.float32, device=dev)
    if packT is None:
        packT = torch.empty(wordsT, dtype=torch.float32, device=dev)
    _flat_f32("radiance_pack_device", "pack", pack, words)
    _flat_f32("radiance_pack_device", "packT", packT, wordsT)
    with torch.cuda.device(dev), _timed("radiance_pack_device", 0.0):
        rc = L.isr_radiance_pack_device(*shape, _hp(fr), float(beta), ptr(W), ptr(b), ptr(pack), words * 4, ptr(packT), wordsT * 4,
                                        current_stream(dev))
    check(rc, "isr_radiance_pack_device")
    return pack, packT


def radiance_backward_flops(widths, H: int, Wc: int, C: int) -> float:
    """Multiply-adds x 2 of one point through the backward as issued: the forward again, the u pass (every trunk layer but
    the first, W1's trunk columns and W2) and the dW pass (W1's direction columns included)."""
    w = [int(v) for v in widths]
    f = radiance_flops(w, H, Wc, C)
    u = 2.0 * (sum(a * b for a, b in zip(w[:-1], w[1:])) + w[-1] * int(Wc) + int(Wc) * int(C) + w[-1])
    return 2.0 * f + u + 2.0 * int(Wc) * 6 * int(H)


def radiance_backward(pack: torch.Tensor, packT: torch.Tensor, widths, H: int, Wc: int, C: int, origins: torch.Tensor,
                      directions: torch.Tensor, lengths: torch.Tensor, d_densities: torch.Tensor | None,
                      d_colours: torch.Tensor | None, need=(True, True), slab: int | None = None,
                      workspace_buf: torch.Tensor | None = None):
    """isr_radiance_backward: the bundle origins (N,3), directions (N,3), lengths (N,P) and the upstream gradients
    d_densities (N,P) and d_colours (N,P,C) f32 (either None: zeros) -> (dW, db) flat in isr_radiance_pack's layout
    (radiance_param_sizes), every entry written; need: which of the two to compute (the other is None).  The forward is
    recomputed from the rays; pack and packT are radiance_pack_device's.  slab: work through the points this many at a time
    (a multiple of the chain length; tests) instead of the default; workspace_buf: a contiguous device buffer to use instead
    of the cached one (tests).  Nothing synchronises."""
    dev = require_cuda(pack, packT, origins, directions, lengths, d_densities, d_colours, workspace_buf)
    N, P, _ = _ray_bundle("radiance_backward", origins, directions, lengths, 0.0)
    C = int(C)
    for what, t, shape in (("d_densities", d_densities, (N, P)), ("d_colours", d_colours, (N, P, C))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"radiance_backward: {what} must be contiguous {shape} float32, got {tuple(t.shape)} {t.dtype}")
    nw, nb = radiance_param_sizes(widths, H, Wc, C)
    shape, _keep = _radiance_shape(widths, H, Wc, C)
    L = lib()
    if workspace_buf is not None:
        ws, ws_bytes = workspace_buf, workspace_buf.numel() * workspace_buf.element_size()
    elif slab is None:
        ws_bytes = L.isr_radiance_grad_workspace_bytes(*shape, N, P)
        ws = workspace(dev, ws_bytes, "radiance_grad") if ws_bytes else None
    else:
        chain = L.isr_radiance_grad_geometry(0)
        if slab < chain or slab % chain:
            raise ValueError(f"radiance_backward: slab {slab} is not a multiple of the chain length {chain}")
        ws_bytes = L.isr_radiance_grad_workspace_bytes(*shape, int(slab), 1)      # `slab` points, a ray each: the most rays
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    if ws_bytes == 0:
        check(-1, "isr_radiance_grad_workspace_bytes")
    dW = torch.empty(nw, dtype=torch.float32, device=dev) if need[0] else None
    db = torch.empty(nb, dtype=torch.float32, device=dev) if need[1] else None
    with torch.cuda.device(dev), _timed("radiance_backward", float(N) * P * radiance_backward_flops(widths, H, Wc, C)):
        rc = L.isr_radiance_backward(ptr(pack), pack.numel() * pack.element_size(), ptr(packT), packT.numel() * packT.element_size(),
                                     *shape, ptr(origins), ptr(directions), ptr(lengths), N, P, ptr(d_densities), ptr(d_colours),
                                     ptr(dW), ptr(db), ptr(ws), ws_bytes, current_stream(dev))
    check(rc, "isr_radiance_backward")
    return dW, db


def radiance_backward_host(pack_host, widths, H: int, Wc: int, C: int, origins, directions, lengths, d_densities=None,
                           d_colours=None, need=(True, True)):
    """isr_radiance_backward_host: radiance_backward as host code over NumPy arrays (pack_host: isr_radiance_pack's words, e.g.
    RadianceField.rpack_host).  For tests."""
    pack_host = np.ascontiguousarray(pack_host, np.float32)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
    ln = np.ascontiguousarray(lengths, np.float32)
    N, P = ln.shape
    dd = None if d_densities is None else np.ascontiguousarray(d_densities, np.float32)
    dc = None if d_colours is None else np.ascontiguousarray(d_colours, np.float32)
    if o.shape[0] != N or d.shape[0] != N or (dd is not None and dd.shape != (N, P)) or (dc is not None and dc.shape != (N, P, int(C))):
        raise ValueError("radiance_backward_host: the shapes of the bundle and the upstream gradients do not agree")
    nw, nb = radiance_param_sizes(widths, H, Wc, C)
    shape, _keep = _radiance_shape(widths, H, Wc, C)
    dW = np.empty(nw, np.float32) if need[0] else None
    db = np.empty(nb, np.float32) if need[1] else None
    check(lib().isr_radiance_backward_host(_hp(pack_host), pack_host.nbytes, *shape, _hp(o), _hp(d), _hp(ln), N, P, _hp(dd), _hp(dc),
                                           _hp(dW), _hp(db)), "isr_radiance_backward_host")
    return dW, db


def radiance_grad_slopes_host(z, beta: float):
    """isr_radiance_grad_slopes_host: (slope32(z, beta), dexp32(z)) of every element of a NumPy f32 array.  For tests."""
    z = np.ascontiguousarray(z, np.float32)
    sl, de = np.empty_like(z), np.empty_like(z)
    check(lib().isr_radiance_grad_slopes_host(_hp(z), z.size, float(beta), _hp(sl), _hp(de)), "isr_radiance_grad_slopes_host")
    return sl, de


# ---- training batches (include/isr_augment.h)
AUGMENT_MAX_SAMPLE = 4096
AUGMENT_MAX_VIEW_ROWS = 1 << 20


def _augment_image_params(name: str, B: int, M, rect, tra, tra1, border, mean, std):
    """The host arrays of isr_augment_images: M (B, 2, 3) f64; rect (B, 4), tra, tra1, border (B, 2) i32 or None; mean, std (3,) f32."""
    Mh = np.ascontiguousarray(np.asarray(M, np.float64).reshape(-1))
    if Mh.size != 6 * B:
        raise ValueError(f"{name}: M must be ({B}, 2, 3), got {np.shape(M)}")

    def ints(a, cols, what):
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1))
        if a.size != cols * B or (np.abs(a) >= 2 ** 31).any():
            raise ValueError(f"{name}: {what} must be ({B}, {cols}) and fit int32")
        return a.astype(np.int32)

    mu, sd = np.ascontiguousarray(mean, np.float32).reshape(-1), np.ascontiguousarray(std, np.float32).reshape(-1)
    if mu.size != 3 or sd.size != 3:
        raise ValueError(f"{name}: mean and std must hold 3 values")
    return Mh, ints(rect, 4, "rect"), ints(tra, 2, "tra"), ints(tra1, 2, "tra1"), ints(border, 2, "border"), mu, sd


def _augment_image_shapes(name: str, rgb, mask, orig_mask, canvas) -> tuple[int, int, int]:
    if rgb.ndim != 4 or rgb.shape[3] != 3 or min(rgb.shape) < 1:
        raise ValueError(f"{name}: rgb must be (B, H, W, 3) and not empty, got {tuple(rgb.shape)}")
    B, H, W, _ = rgb.shape
    for what, m in (("mask", mask), ("orig_mask", orig_mask)):
        if m is not None and tuple(m.shape) != (B, H, W):
            raise ValueError(f"{name}: {what} must be ({B}, {H}, {W}), got {tuple(m.shape)}")
    if canvas is not None and tuple(canvas.shape) != (B, H, W, 3):
        raise ValueError(f"{name}: canvas must be ({B}, {H}, {W}, 3), got {tuple(canvas.shape)}")
    return int(B), int(H), int(W)


def augment_images(rgb: torch.Tensor, mask: torch.Tensor, M, *, orig_mask: torch.Tensor | None = None,
                   canvas: torch.Tensor | None = None, rect=None, tra=None, tra1=None, border=None, mean=IMAGENET_MEAN,
                   std=IMAGENET_STD):
    """isr_augment_images: rgb (B, H, W, 3) f32, mask (B, H, W) u8 holding 0/1, orig_mask likewise (None: mask), canvas
    (B, H, W, 3) f32 or None (zeros) on the device; M (B, 2, 3) f64, rect (B, 4) = (x, y, w, h), tra, tra1 (B, 2) and border
    (B, 2) = (kh, kw) on the host (None: no rectangle, zero shifts, no border) -> (rgb_out (B, H, W, 3), mask_orig_out (B, H, W),
    mask_out (B, H, W)) f32 on the device: generateImages' two warps, paste and border blanking, then dataGen.normalize.
    Nothing synchronises."""
    dev = require_cuda(rgb, mask, orig_mask, canvas)
    if rgb.dtype != torch.float32 or mask.dtype != torch.uint8 or (orig_mask is not None and orig_mask.dtype != torch.uint8) \
            or (canvas is not None and canvas.dtype != torch.float32):
        raise ValueError("augment_images: rgb and canvas must be float32, the masks uint8")
    B, H, W = _augment_image_shapes("augment_images", rgb, mask, orig_mask, canvas)
    rgb, mask = rgb.contiguous(), mask.contiguous()
    orig = mask if orig_mask is None else orig_mask.contiguous()
    canvas = None if canvas is None else canvas.contiguous()
    Mh, rc_, t_, t1_, bd_, mu, sd = _augment_image_params("augment_images", B, M, rect, tra, tra1, border, mean, std)
    rgb_out = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    mask_orig_out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    mask_out = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("augment_images", float(B) * H * W):
        rc = lib().isr_augment_images(ptr(rgb), ptr(mask), ptr(orig), ptr(canvas), B, H, W, _hp(rc_), _hp(Mh), _hp(t_), _hp(t1_),
                                      _hp(bd_), _hp(mu), _hp(sd), ptr(rgb_out), ptr(mask_orig_out), ptr(mask_out),
                                      current_stream(dev))
    check(rc, "isr_augment_images")
    return rgb_out, mask_orig_out, mask_out


def augment_images_host(rgb, mask, M, *, orig_mask=None, canvas=None, rect=None, tra=None, tra1=None, border=None,
                        mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """isr_augment_images_host: the same images as host code over NumPy arrays.  For tests."""
    rgb, mask = np.ascontiguousarray(rgb, np.float32), np.ascontiguousarray(mask, np.uint8)
    orig = mask if orig_mask is None else np.ascontiguousarray(orig_mask, np.uint8)
    canvas = None if canvas is None else np.ascontiguousarray(canvas, np.float32)
    B, H, W = _augment_image_shapes("augment_images_host", rgb, mask, orig, canvas)
    Mh, rc_, t_, t1_, bd_, mu, sd = _augment_image_params("augment_images_host", B, M, rect, tra, tra1, border, mean, std)
    rgb_out, mask_orig_out, mask_out = np.empty((B, H, W, 3), np.float32), np.empty((B, H, W), np.float32), np.empty((B, H, W), np.float32)
    check(lib().isr_augment_images_host(_hp(rgb), _hp(mask), _hp(orig), _hp(canvas), B, H, W, _hp(rc_), _hp(Mh), _hp(t_), _hp(t1_),
                                        _hp(bd_), _hp(mu), _hp(sd), _hp(rgb_out), _hp(mask_orig_out), _hp(mask_out)),
          "isr_augment_images_host")
    return rgb_out, mask_orig_out, mask_out


@dataclass
class AugmentedRays:
    """One set's sample: xys (B, S, 2) the remapped locations, pos (B, S, 3), index (B, S) i32 (the row in the view, -1 past the
    count), count (B,) i32; rows past the count are zeros."""
    xys: "torch.Tensor | np.ndarray"
    pos: "torch.Tensor | np.ndarray"
    index: "torch.Tensor | np.ndarray"
    count: "torch.Tensor | np.ndarray"


def _augment_ray_params(name: str, front, back, view_ids, rot, t, S: int):
    """Checks of isr_augment_rays -> (B, V, host arrays offsets_front, offsets_back or None, view_ids, rot, t).  front / back:
    (xys (n, 2), pos (n, 3), offsets (V + 1))."""
    ids = np.ascontiguousarray(np.asarray(view_ids, np.int64).reshape(-1))
    B = ids.size
    rot_, t_ = np.ascontiguousarray(rot, np.float32).reshape(-1), np.ascontiguousarray(t, np.float32).reshape(-1)
    if B < 1 or rot_.size != 4 * B or t_.size != 2 * B:
        raise ValueError(f"{name}: view_ids (B,), rot (B, 4) and t (B, 2) with B >= 1, got {ids.shape}, {np.shape(rot)}, {np.shape(t)}")
    if not 1 <= int(S) <= AUGMENT_MAX_SAMPLE:
        raise ValueError(f"{name}: S = {S} outside 1..{AUGMENT_MAX_SAMPLE}")
    offs, V = [], None
    for what, bank in (("front", front), ("back", back)):
        if bank is None:
            offs.append(None)
            continue
        xys, pos, off = bank
        off = np.ascontiguousarray(np.asarray(off, np.int64).reshape(-1))
        if V is None:
            V = off.size - 1
        if off.size - 1 != V or V < 1 or off[0] != 0 or (np.diff(off) < 0).any():
            raise ValueError(f"{name}: the {what} offsets must be (V + 1,) from 0 and non-decreasing, the same V for both sets")
        n = int(off[-1])
        if xys.ndim != 2 or xys.shape[1] != 2 or pos.ndim != 2 or pos.shape[1] != 3 or xys.shape[0] != n or pos.shape[0] != n:
            raise ValueError(f"{name}: the {what} bank must be xys ({n}, 2) and pos ({n}, 3), got {tuple(xys.shape)} and {tuple(pos.shape)}")
        offs.append(off)
    if (ids < 0).any() or (ids >= V).any():
        raise ValueError(f"{name}: view ids outside 0..{V - 1}")
    return B, V, offs[0], offs[1], ids.astype(np.int32), rot_, t_


def augment_rays(front, view_ids, rot, t, S: int, seed: int, back=None):
    """isr_augment_rays: front = (xys (sum n, 2) f32, pos (sum n, 3) f32 on the device, offsets (V + 1) on the host), back
    likewise or None; view_ids (B,), rot (B, 4) = (m00, m01, m10, m11) f32 and t (B, 2) f32 on the host -> AugmentedRays of the
    front set, or (front, back): getNerfSamples' remap and inside filter, and the min(S, m) candidates with the smallest
    Philox keys of (seed, view id, set, row), in key order.  Nothing synchronises."""
    dev = require_cuda(front[0], front[1], *(back[:2] if back is not None else ()))
    B, V, off_f, off_b, ids, rot_, t_ = _augment_ray_params("augment_rays", front, back, view_ids, rot, t, S)
    S = int(S)
    sets, outs, args = [], [], []
    for bank in (front, back):
        if bank is None:
            args += [None, None, None, None]
            sets.append((None, None))
            continue
        xys, pos = bank[0], bank[1]
        if xys.dtype != torch.float32 or pos.dtype != torch.float32:
            raise ValueError("augment_rays: float32 banks only")
        if xys.shape[0] == 0:                                                         # an empty bank still needs an address
            xys, pos = torch.zeros((1, 2), dtype=torch.float32, device=dev), torch.zeros((1, 3), dtype=torch.float32, device=dev)
        sets.append((xys.contiguous(), pos.contiguous()))
        o = AugmentedRays(torch.empty((B, S, 2), dtype=torch.float32, device=dev), torch.empty((B, S, 3), dtype=torch.float32, device=dev),
                          torch.empty((B, S), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        outs.append(o)
        args += [ptr(o.xys), ptr(o.pos), ptr(o.index), ptr(o.count)]
    with torch.cuda.device(dev), _timed("augment_rays", float(B) * S):
        rc = lib().isr_augment_rays(ptr(sets[0][0]), ptr(sets[0][1]), _hp(off_f), ptr(sets[1][0]), ptr(sets[1][1]), _hp(off_b), V,
                                    _hp(ids), _hp(rot_), _hp(t_), B, S, int(seed) & 0xFFFFFFFFFFFFFFFF, *args, current_stream(dev))
    check(rc, "isr_augment_rays")
    return outs[0] if back is None else (outs[0], outs[1])


def augment_rays_host(front, view_ids, rot, t, S: int, seed: int, back=None):
    """isr_augment_rays_host: the same samples as host code over NumPy arrays.  For tests."""
    B, V, off_f, off_b, ids, rot_, t_ = _augment_ray_params("augment_rays_host", front, back, view_ids, rot, t, S)
    S = int(S)
    sets, outs, args = [], [], []
    for bank in (front, back):
        if bank is None:
            args += [None, None, None, None]
            sets.append((None, None))
            continue
        xys, pos = np.ascontiguousarray(bank[0], np.float32), np.ascontiguousarray(bank[1], np.float32)
        if xys.shape[0] == 0:
            xys, pos = np.zeros((1, 2), np.float32), np.zeros((1, 3), np.float32)
        sets.append((xys, pos))
        o = AugmentedRays(np.empty((B, S, 2), np.float32), np.empty((B, S, 3), np.float32), np.empty((B, S), np.int32),
                          np.empty(B, np.int32))
        outs.append(o)
        args += [_hp(o.xys), _hp(o.pos), _hp(o.index), _hp(o.count)]
    check(lib().isr_augment_rays_host(_hp(sets[0][0]), _hp(sets[0][1]), _hp(off_f), _hp(sets[1][0]), _hp(sets[1][1]), _hp(off_b), V,
                                      _hp(ids), _hp(rot_), _hp(t_), B, S, int(seed) & 0xFFFFFFFFFFFFFFFF, *args),
          "isr_augment_rays_host")
    return outs[0] if back is None else (outs[0], outs[1])


# ---- the colour augmentation pass (include/isr_color_aug.h)
# isr_color_program, 120 bytes: the gates, the jitter order, the factors and the noise key of one image
COLOR_PROGRAM = np.dtype([("pass", "<i4"), ("jitter", "<i4"), ("order", "<i4", (4,)), ("rbc", "<i4"), ("ksize", "<i4"),
                          ("iso", "<i4"), ("clahe", "<i4"), ("brightness", "<f8"), ("contrast", "<f8"), ("saturation", "<f8"),
                          ("hue", "<f8"), ("alpha", "<f8"), ("beta", "<f8"), ("color_shift", "<f8"), ("intensity", "<f8"),
                          ("clip_limit", "<f8"), ("noise_key", "<u8")])


def color_aug_geometry() -> dict:
    """isr_color_aug_geometry: the per-pixel workgroup's threads, the images per launch, the most launches per 16 images and the
    program's bytes."""
    L = lib()
    return {k: int(L.isr_color_aug_geometry(i)) for i, k in enumerate(("threads", "images_per_launch", "max_launches", "program_bytes"))}


def color_programs(B: int) -> np.ndarray:
    """B programs with every gate off and neutral factors: what a hand-built program starts from."""
    p = np.zeros(int(B), COLOR_PROGRAM)
    p["order"] = (0, 1, 2, 3)
    for k in ("brightness", "contrast", "saturation", "alpha", "clip_limit"):
        p[k] = 1.0
    return p


def _color_aug_args(name: str, image, programs, select, under, border, border_mask, mean, std):
    """Shape checks of isr_augment_color -> (B, H, W, programs, border, mean3, std3); the library checks the limits."""
    if image.ndim != 4 or image.shape[3] != 3 or min(image.shape) < 1:
        raise ValueError(f"{name}: image must be (B, H, W, 3) and not empty, got {tuple(image.shape)}")
    B, H, W, _ = (int(v) for v in image.shape)
    progs = np.ascontiguousarray(programs)
    if progs.dtype != COLOR_PROGRAM or progs.shape != (B,):
        raise ValueError(f"{name}: programs must be ({B},) of ops.COLOR_PROGRAM, got {progs.shape} of {progs.dtype}")
    for what, t, shape in (("select", select, (B, H, W)), ("under", under, (B, H, W, 3)), ("border_mask", border_mask, (B, H, W))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name}: {what} must be {shape}, got {tuple(t.shape)}")
    if under is not None and select is None:
        raise ValueError(f"{name}: under needs select")
    if (border is None) != (border_mask is None):
        raise ValueError(f"{name}: border and border_mask go together")
    if (mean is None) != (std is None):
        raise ValueError(f"{name}: mean and std go together")
    bd = None
    if border is not None:
        bd = np.ascontiguousarray(np.asarray(border, np.int64).reshape(-1))
        if bd.size != 2 * B or (np.abs(bd) >= 2 ** 31).any():
            raise ValueError(f"{name}: border must be ({B}, 2) and fit int32")
        bd = bd.astype(np.int32)
    mu = sd = None
    if mean is not None:
        mu, sd = np.ascontiguousarray(mean, np.float32).reshape(-1), np.ascontiguousarray(std, np.float32).reshape(-1)
        if mu.size != 3 or sd.size != 3:
            raise ValueError(f"{name}: mean and std must hold 3 values")
    return B, H, W, progs, bd, mu, sd


def augment_color(image: torch.Tensor, programs, *, select: torch.Tensor | None = None, under: torch.Tensor | None = None,
                  border=None, border_mask: torch.Tensor | None = None, mean=None, std=None) -> torch.Tensor:
    """isr_augment_color: image (B, H, W, 3) f32 in [0, 1] on the device, programs (B,) of COLOR_PROGRAM on the host -> (B, H, W, 3)
    f32: the albumentations pass of augment.py:344-350 as include/isr_color_aug.h states it.  select (B, H, W) f32 holding 0/1
    with under (B, H, W, 3) or None: the pass's pixels where select == 1, under (zeros) elsewhere.  border (B, 2) = (kh, kw) on
    the host with border_mask (B, H, W), and mean / std: augment_images' blanking and normalize.  At most eight
    launches per 16 images, nothing synchronises."""
    dev = require_cuda(image, select, under, border_mask)
    if any(t is not None and t.dtype != torch.float32 for t in (image, select, under, border_mask)):
        raise ValueError("augment_color: image, select, under and border_mask must be float32")
    B, H, W, progs, bd, mu, sd = _color_aug_args("augment_color", image, programs, select, under, border, border_mask, mean, std)
    c = lambda t: None if t is None else t.contiguous()
    image, select, under, border_mask = c(image), c(select), c(under), c(border_mask)
    ws = workspace(dev, lib().isr_color_aug_workspace_bytes(B, H, W), "color_aug")      # 0 bytes: a shape the call refuses
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("augment_color", float(B) * H * W):
        rc = lib().isr_augment_color(ptr(image), B, H, W, _hp(progs), ptr(select), ptr(under), _hp(bd), ptr(border_mask), _hp(mu),
                                     _hp(sd), ptr(out), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_augment_color")
    return out


def augment_color_host(image, programs, *, select=None, under=None, border=None, border_mask=None, mean=None, std=None):
    """isr_augment_color_host: the same pass as host code over NumPy arrays.  For tests."""
    c = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    image, select, under, border_mask = c(image), c(select), c(under), c(border_mask)
    B, H, W, progs, bd, mu, sd = _color_aug_args("augment_color_host", image, programs, select, under, border, border_mask, mean, std)
    out = np.empty((B, H, W, 3), np.float32)
    check(lib().isr_augment_color_host(_hp(image), B, H, W, _hp(progs), _hp(select), _hp(under), _hp(bd), _hp(border_mask), _hp(mu),
                                       _hp(sd), _hp(out)), "isr_augment_color_host")
    return out


def color_aug_draws_host(noise_key: int, n: int, lam: float):
    """isr_color_aug_draws_host: ISONoise's draws of pixels 0 .. n-1 at a given lambda -> (k (n,) i32, z (n,) f64).  For tests."""
    k, z = np.empty(int(n), np.int32), np.empty(int(n), np.float64)
    check(lib().isr_color_aug_draws_host(int(noise_key) & 0xFFFFFFFFFFFFFFFF, int(n), float(lam), _hp(k), _hp(z)),
          "isr_color_aug_draws_host")
    return k, z


# ---- the fused multi-tensor Adam (include/isr_adam.h)
ADAM_MAX_GROUPS = 8
ADAM_CHUNK = 4096
# isr_adam_tensor, 48 bytes: the addresses of p, g, m, v, the element count, the group and the step slot
ADAM_TENSOR = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("group", "<i4"), ("slot", "<i4")])


def adam_geometry() -> dict:
    """isr_adam_geometry: the descriptor's bytes, the chunk's elements, the workgroup's threads and the most groups, as built."""
    L = lib()
    return {k: int(L.isr_adam_geometry(i)) for i, k in enumerate(("tensor_bytes", "chunk", "threads", "max_groups"))}


def adam_groups(groups) -> np.ndarray:
    """(G, 6) f64 rows of (lr, beta1, beta2, eps, weight_decay, ramp) from a sequence of such rows."""
    g = np.ascontiguousarray(np.asarray(groups, np.float64))
    if g.ndim != 2 or g.shape[1] != 6:
        raise ValueError(f"adam: groups must be (G, 6) = (lr, beta1, beta2, eps, weight_decay, ramp), got {g.shape}")
    return g


def adam_table_host(table: np.ndarray, G: int, n_slots: int):
    """isr_adam_table_host: checks a host table of ADAM_TENSOR rows -> (chunk_start (T + 1) i32, chunks)."""
    if table.dtype != ADAM_TENSOR or table.ndim != 1 or not table.flags.c_contiguous:
        raise ValueError("adam_table_host: table must be a contiguous 1-d array of ops.ADAM_TENSOR")
    T = int(table.shape[0])
    chunk_start = np.zeros(T + 1, np.int32)
    chunks = ctypes.c_int64(0)
    check(lib().isr_adam_table_host(_hp(table) if T else None, T, int(G), int(n_slots), _hp(chunk_start), ctypes.byref(chunks)),
          "isr_adam_table_host")
    return chunk_start, int(chunks.value)


def adam_step(table: torch.Tensor, chunk_start: torch.Tensor, T: int, chunks: int, groups: np.ndarray, steps: torch.Tensor,
              zero_grads: bool = False) -> None:
    """isr_adam_step: table (the bytes of T ADAM_TENSOR rows) and chunk_start (T + 1) i32 on the device, copies of what
    adam_table_host accepted; groups (G, 6) f64 on the host; steps i64 on the device.  Two launches, nothing synchronises."""
    dev = require_cuda(table, chunk_start, steps)
    if steps.dtype != torch.int64 or chunk_start.dtype != torch.int32 or not steps.is_contiguous():
        raise ValueError("adam_step: steps must be contiguous int64, chunk_start int32")
    groups = adam_groups(groups)
    with torch.cuda.device(dev), _timed("adam_step", float(chunks) * ADAM_CHUNK):
        rc = lib().isr_adam_step(ptr(table), ptr(chunk_start), int(T), int(chunks), _hp(groups), int(groups.shape[0]), ptr(steps),
                                 int(bool(zero_grads)), current_stream(dev))
    check(rc, "isr_adam_step")


def adam_zero_grads(table: torch.Tensor, chunk_start: torch.Tensor, T: int, chunks: int) -> None:
    """isr_adam_zero_grads: +0 to every gradient of the table, one launch."""
    dev = require_cuda(table, chunk_start)
    with torch.cuda.device(dev), _timed("adam_zero_grads", float(chunks) * ADAM_CHUNK):
        rc = lib().isr_adam_zero_grads(ptr(table), ptr(chunk_start), int(T), int(chunks), current_stream(dev))
    check(rc, "isr_adam_zero_grads")


def adam_step_host(params, grads, exp_avgs, exp_avg_sqs, group_of, groups, steps: np.ndarray, slots=None,
                   zero_grads: bool = False) -> None:
    """isr_adam_step_host: one step, in place, over lists of 1-d float32 NumPy arrays (views allowed: their addresses are
    used as they are); group_of: each tensor's row of groups (G, 6); steps: int64 counters, tensor i using steps[slots[i]]
    (slots None: i).  For tests."""
    T = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(group_of) == T):
        raise ValueError("adam_step_host: the lists differ in length")
    if steps.dtype != np.int64 or not steps.flags.c_contiguous:
        raise ValueError("adam_step_host: steps must be contiguous int64")
    slots = list(range(T)) if slots is None else list(slots)
    table = np.zeros(T, ADAM_TENSOR)
    for i, arrays in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        n = arrays[0].size
        for name, a in zip("pgmv", arrays):
            if a.dtype != np.float32 or a.size != n or (a.size > 1 and a.ndim == 1 and a.strides[0] != 4) \
                    or (a.ndim != 1 and not a.flags.c_contiguous) or not a.flags.writeable:
                raise ValueError(f"adam_step_host: tensor {i}: {name} must be writeable dense float32 of {n} elements")
            table[name][i] = a.ctypes.data
        table["n"][i], table["group"][i], table["slot"][i] = n, group_of[i], slots[i]
    groups = adam_groups(groups)
    check(lib().isr_adam_step_host(_hp(table) if T else None, T, _hp(groups), int(groups.shape[0]), _hp(steps), int(steps.size),
                                   int(bool(zero_grads))), "isr_adam_step_host")


def adam_scalars_host(group, t: int):
    """isr_adam_scalars_host: group = (lr, beta1, beta2, eps, weight_decay, ramp), t the 1-based step ->
    dict(lr_t, beta1_t, beta2_t as f64; step, r as f32)."""
    g = adam_groups([group])
    out4, out2 = np.zeros(4, np.float64), np.zeros(2, np.float32)
    check(lib().isr_adam_scalars_host(_hp(g), int(t), _hp(out4), _hp(out2)), "isr_adam_scalars_host")
    return {"lr_t": float(out4[0]), "beta1_t": float(out4[1]), "beta2_t": float(out4[2]), "step": out2[0], "r": out2[1]}


# ---- the ray losses and their gradients (include/isr_ray_losses.h)
def ray_losses_geometry() -> dict:
    """isr_ray_losses_geometry: the rays of a distortion workgroup, the lanes that share a ray, the leaves of a reduction tree
    (the rays of a render-loss workgroup) and the largest P."""
    L = lib()
    return {k: int(L.isr_ray_losses_geometry(i)) for i, k in enumerate(("group_rays", "lanes", "reduce", "max_p"))}


def _distortion_shape(name: str, lengths, weights):
    """-> (N, P) of lengths (N, P) and weights (N, P); the library checks the limits."""
    if lengths.ndim != 2 or tuple(weights.shape) != tuple(lengths.shape):
        raise ValueError(f"{name}: lengths (N, P) and weights (N, P) expected, got {tuple(lengths.shape)} and {tuple(weights.shape)}")
    return int(lengths.shape[0]), int(lengths.shape[1])


def _ray_losses_workspace(dev, nbytes: int, what: str) -> torch.Tensor:
    if nbytes == 0:
        check(-1, what)
    return workspace(dev, nbytes, "ray_losses")


def distortion_forward(lengths: torch.Tensor, weights: torch.Tensor, want_ray_loss: bool = True):
    """isr_distortion_forward: lengths (N, P), weights (N, P) contiguous f32 on the device -> (ray_loss (N) or None, loss (0-d)):
    nutil.mip360loss as include/isr_ray_losses.h states it.  No (P, P) array is made; nothing synchronises."""
    dev = _contrastive_device("distortion_forward", lengths, weights)
    N, P = _distortion_shape("distortion_forward", lengths, weights)
    ws = _ray_losses_workspace(dev, lib().isr_distortion_workspace_bytes(N, P), "isr_distortion_workspace_bytes")
    ray_loss = torch.empty((N,), dtype=torch.float32, device=dev) if want_ray_loss else None
    loss = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("distortion_forward", 3.0 * N * P * P):
        rc = lib().isr_distortion_forward(ptr(lengths), ptr(weights), N, P, ptr(ray_loss), ptr(loss), ptr(ws), ws.numel(),
                                          current_stream(dev))
    check(rc, "isr_distortion_forward")
    return ray_loss, loss


def distortion_backward(lengths: torch.Tensor, weights: torch.Tensor, upstream: torch.Tensor) -> torch.Tensor:
    """isr_distortion_backward: dweights (N, P) of distortion_forward's loss; upstream: a device tensor of one f32, read on the
    device.  One launch, nothing synchronises."""
    dev = _contrastive_device("distortion_backward", lengths, weights, upstream)
    N, P = _distortion_shape("distortion_backward", lengths, weights)
    if upstream.numel() != 1:
        raise ValueError("distortion_backward: upstream must hold one value")
    dweights = torch.empty_like(weights)
    with torch.cuda.device(dev), _timed("distortion_backward", 3.0 * N * P * P):
        rc = lib().isr_distortion_backward(ptr(lengths), ptr(weights), N, P, ptr(upstream), ptr(dweights), current_stream(dev))
    check(rc, "isr_distortion_backward")
    return dweights


def distortion_forward_host(lengths, weights, want_ray_loss: bool = True):
    """isr_distortion_forward_host: distortion_forward as host code over NumPy arrays.  For tests."""
    lengths, weights = _contrastive_host("distortion_forward_host", lengths, weights)
    N, P = _distortion_shape("distortion_forward_host", lengths, weights)
    ray_loss = np.empty((N,), np.float32) if want_ray_loss else None
    loss = np.empty((), np.float32)
    check(lib().isr_distortion_forward_host(_hp(lengths), _hp(weights), N, P, _hp(ray_loss), _hp(loss)), "isr_distortion_forward_host")
    return ray_loss, loss


def distortion_backward_host(lengths, weights, upstream: float = 1.0):
    """isr_distortion_backward_host: distortion_backward as host code over NumPy arrays.  For tests."""
    lengths, weights = _contrastive_host("distortion_backward_host", lengths, weights)
    N, P = _distortion_shape("distortion_backward_host", lengths, weights)
    up = np.array([upstream], np.float32)
    dweights = np.empty_like(weights)
    check(lib().isr_distortion_backward_host(_hp(lengths), _hp(weights), N, P, _hp(up), _hp(dweights)), "isr_distortion_backward_host")
    return dweights


def _render_loss_shape(name: str, rendered, target_images, target_silhouettes, xys):
    """-> (B, n, F, H, W) of rendered (B, n, F+1), target_images (B, H, W, F), target_silhouettes (B, H, W), xys (B, n, 2)."""
    ok = rendered.ndim == 3 and target_images.ndim == 4 and rendered.shape[2] == target_images.shape[3] + 1 \
        and tuple(target_silhouettes.shape) == tuple(target_images.shape[:3]) and rendered.shape[0] == target_images.shape[0] \
        and tuple(xys.shape) == (rendered.shape[0], rendered.shape[1], 2)
    if not ok:
        raise ValueError(f"{name}: rendered (B, n, F+1), target_images (B, H, W, F), target_silhouettes (B, H, W), xys (B, n, 2) "
                         f"expected, got {tuple(rendered.shape)}, {tuple(target_images.shape)}, {tuple(target_silhouettes.shape)}, "
                         f"{tuple(xys.shape)}")
    return (int(rendered.shape[0]), int(rendered.shape[1]), int(target_images.shape[3]), int(target_images.shape[1]),
            int(target_images.shape[2]))


def render_loss_forward(rendered: torch.Tensor, target_images: torch.Tensor, target_silhouettes: torch.Tensor, xys: torch.Tensor,
                        scaling: float = 0.1) -> torch.Tensor:
    """isr_render_loss_forward: contiguous f32 device tensors -> out (2): the means of nutil.huber(...).abs() of the colours and
    of the opacity of a render against its targets at the rays (trainNerfFine.py:314-326).  Nothing synchronises."""
    dev = _contrastive_device("render_loss_forward", rendered, target_images, target_silhouettes, xys)
    B, n, F, H, W = _render_loss_shape("render_loss_forward", rendered, target_images, target_silhouettes, xys)
    ws = _ray_losses_workspace(dev, lib().isr_render_loss_workspace_bytes(B, n), "isr_render_loss_workspace_bytes")
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("render_loss_forward", 8.0 * B * n * (F + 1)):
        rc = lib().isr_render_loss_forward(ptr(rendered), ptr(target_images), ptr(target_silhouettes), ptr(xys), B, n, F, H, W,
                                           float(scaling), ptr(out), ptr(ws), ws.numel(), current_stream(dev))
    check(rc, "isr_render_loss_forward")
    return out


def render_loss_backward(rendered: torch.Tensor, target_images: torch.Tensor, target_silhouettes: torch.Tensor, xys: torch.Tensor,
                         upstream: torch.Tensor, scaling: float = 0.1) -> torch.Tensor:
    """isr_render_loss_backward: drendered (B, n, F+1); upstream: a device tensor of two f32 (colour, silhouette), read on the
    device.  One launch, nothing synchronises."""
    dev = _contrastive_device("render_loss_backward", rendered, target_images, target_silhouettes, xys, upstream)
    B, n, F, H, W = _render_loss_shape("render_loss_backward", rendered, target_images, target_silhouettes, xys)
    if upstream.numel() != 2:
        raise ValueError("render_loss_backward: upstream must hold two values")
    drendered = torch.empty_like(rendered)
    with torch.cuda.device(dev), _timed("render_loss_backward", 8.0 * B * n * (F + 1)):
        rc = lib().isr_render_loss_backward(ptr(rendered), ptr(target_images), ptr(target_silhouettes), ptr(xys), B, n, F, H, W,
                                            float(scaling), ptr(upstream), ptr(drendered), current_stream(dev))
    check(rc, "isr_render_loss_backward")
    return drendered


def render_loss_forward_host(rendered, target_images, target_silhouettes, xys, scaling: float = 0.1):
    """isr_render_loss_forward_host: render_loss_forward as host code over NumPy arrays.  For tests."""
    a = _contrastive_host("render_loss_forward_host", rendered, target_images, target_silhouettes, xys)
    B, n, F, H, W = _render_loss_shape("render_loss_forward_host", *a)
    out = np.empty((2,), np.float32)
    check(lib().isr_render_loss_forward_host(*map(_hp, a), B, n, F, H, W, float(scaling), _hp(out)), "isr_render_loss_forward_host")
    return out


def render_loss_backward_host(rendered, target_images, target_silhouettes, xys, upstream=(1.0, 1.0), scaling: float = 0.1):
    """isr_render_loss_backward_host: render_loss_backward as host code over NumPy arrays.  For tests."""
    a = _contrastive_host("render_loss_backward_host", rendered, target_images, target_silhouettes, xys)
    B, n, F, H, W = _render_loss_shape("render_loss_backward_host", *a)
    up = np.array(upstream, np.float32)
    drendered = np.empty_like(a[0])
    check(lib().isr_render_loss_backward_host(*map(_hp, a), B, n, F, H, W, float(scaling), _hp(up), _hp(drendered)),
          "isr_render_loss_backward_host")
    return drendered


# ---- sequence ingest (include/isr_ingest.h)
INGEST_SILHOUETTE = {"linear": 0, "nearest": 1}


class IngestedViews(NamedTuple):
    """ops.ingest_views' result: images (n, maxB, maxB, 3) f32, silhouettes (n, maxB, maxB) f32, K (n, 4, 4) f64,
    geom (n, 8) i32 = (x2, y2, w2, h2, hw, hh, side, hs1), status (n,) i32 (1: the frame's square has side 0)."""
    images: object
    silhouettes: object
    K: object
    geom: object
    status: object


def ingest_geometry() -> dict:
    """isr_ingest_geometry: threads per workgroup, frames per blockIdx.z group, launches per call."""
    L = lib()
    return {k: int(L.isr_ingest_geometry(i)) for i, k in enumerate(("threads", "frame_group", "launches"))}


def ingest_strips(H: int, W: int, Cm: int) -> tuple[int, int]:
    """(rows per strip, strips per frame) of the box pass; (0, 0) for a shape the call refuses."""
    L = lib()
    return int(L.isr_ingest_strip_rows(int(H), int(W), int(Cm))), int(L.isr_ingest_strips(int(H), int(W), int(Cm)))


def ingest_workspace_bytes(n: int, H: int, W: int, Cm: int) -> int:
    """isr_ingest_workspace_bytes: the box pass's partial boxes; 0 for a shape the call refuses."""
    return int(lib().isr_ingest_workspace_bytes(int(n), int(H), int(W), int(Cm)))


def _ingest_args(name: str, rgb, mask, K, silhouette):
    """Shape checks of isr_ingest_views -> (n, H, W, Cm, sil_mode); the library checks the limits."""
    if rgb.ndim != 4 or rgb.shape[3] != 3 or min(rgb.shape) < 1:
        raise ValueError(f"{name}: rgb must be (n, H, W, 3) and not empty, got {tuple(rgb.shape)}")
    n, H, W, _ = (int(v) for v in rgb.shape)
    if mask.ndim == 3:
        mask = mask[..., None]
    if mask.ndim != 4 or tuple(mask.shape[:3]) != (n, H, W):
        raise ValueError(f"{name}: mask must be ({n}, {H}, {W}[, Cm]), got {tuple(mask.shape)}")
    if int(np.prod(tuple(K.shape))) != 9 * n:
        raise ValueError(f"{name}: K must be ({n}, 3, 3), got {tuple(K.shape)}")
    if silhouette not in INGEST_SILHOUETTE:
        raise ValueError(f"{name}: silhouette must be 'linear' or 'nearest', got {silhouette!r}")
    return mask, n, H, W, int(mask.shape[3]), INGEST_SILHOUETTE[silhouette]


def ingest_views(rgb: torch.Tensor, mask: torch.Tensor, K: torch.Tensor, max_b: int, offset: int = 10, make_ndc: bool = True,
                 silhouette: str = "linear", workspace_buf: torch.Tensor | None = None) -> IngestedViews:
    """isr_ingest_views: rgb (n, H, W, 3) u8, mask (n, H, W[, Cm]) u8 with Cm in {1, 3} and K (n, 3, 3) f64 on the device ->
    IngestedViews on the device: cowrendersynth.generate_bop_realsamples' gate, box, square canvas, resize to max_b and camera
    as include/isr_ingest.h states them.  Three launches, nothing synchronises; the box never visits the host.
    workspace_buf: a caller's u8 buffer of at least ingest_workspace_bytes(...) (default: the cached one)."""
    dev = require_cuda(rgb, mask, K)
    if rgb.dtype != torch.uint8 or mask.dtype != torch.uint8 or K.dtype != torch.float64:
        raise ValueError("ingest_views: rgb and mask must be uint8, K float64")
    mask, n, H, W, Cm, mode = _ingest_args("ingest_views", rgb, mask, K, silhouette)
    rgb, mask, K = rgb.contiguous(), mask.contiguous(), K.contiguous()
    B = int(max_b)
    Bs = max(B, 0)
    ws = workspace_buf if workspace_buf is not None else workspace(dev, ingest_workspace_bytes(n, H, W, Cm), "ingest")
    images = torch.empty((n, Bs, Bs, 3), dtype=torch.float32, device=dev)
    sil = torch.empty((n, Bs, Bs), dtype=torch.float32, device=dev)
    K_out = torch.empty((n, 4, 4), dtype=torch.float64, device=dev)
    geom = torch.empty((n, 8), dtype=torch.int32, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _timed("ingest_views", float(n) * H * W):
        rc = lib().isr_ingest_views(ptr(rgb), ptr(mask), ptr(K), n, H, W, Cm, B, int(offset), int(bool(make_ndc)), mode, ptr(images),
                                    ptr(sil), ptr(K_out), ptr(geom), ptr(status), ptr(ws), ws.numel() * ws.element_size(),
                                    current_stream(dev))
    check(rc, "isr_ingest_views")
    return IngestedViews(images, sil, K_out, geom, status)


def ingest_views_host(rgb, mask, K, max_b: int, offset: int = 10, make_ndc: bool = True, silhouette: str = "linear") -> IngestedViews:
    """isr_ingest_views_host: the same views as host code over NumPy arrays (the tests' reference, and ingest's device="cpu")."""
    rgb, mask = np.ascontiguousarray(rgb, np.uint8), np.ascontiguousarray(mask, np.uint8)
    K = np.ascontiguousarray(K, np.float64)
    mask, n, H, W, Cm, mode = _ingest_args("ingest_views_host", rgb, mask, K, silhouette)
    mask = np.ascontiguousarray(mask)
    B = int(max_b)
    Bs = max(B, 0)
    images, sil = np.empty((n, Bs, Bs, 3), np.float32), np.empty((n, Bs, Bs), np.float32)
    K_out, geom, status = np.empty((n, 4, 4), np.float64), np.empty((n, 8), np.int32), np.empty((n,), np.int32)
    check(lib().isr_ingest_views_host(_hp(rgb), _hp(mask), _hp(K), n, H, W, Cm, B, int(offset), int(bool(make_ndc)), mode, _hp(images),
                                      _hp(sil), _hp(K_out), _hp(geom), _hp(status)), "isr_ingest_views_host")
    return IngestedViews(images, sil, K_out, geom, status)


def ingest_launch_floor(n: int, H: int, W: int, Cm: int, max_b: int, device) -> None:
    """isr_ingest_launch_floor: the call's three launches with empty kernels (tools/bench_ingest.py)."""
    dev = torch.device(device)
    with torch.cuda.device(dev):
        check(lib().isr_ingest_launch_floor(int(n), int(H), int(W), int(Cm), int(max_b), current_stream(dev)), "isr_ingest_launch_floor")
