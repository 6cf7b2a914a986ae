"""refine_pose() with the reference's signature (pose_refine.py:21-104).

The caller-supplied objects are used exactly as the reference uses them: `renderer.render(obj_idx,
K_crop, R, t[:,None])` for the visible object coordinates, `neural_radiance_field.batched_customForward`
for their key descriptors, `obj_.scale / .offset / .diameter`.  What runs in HIP kernels: the
log-sum-exp denominator image (K1's `lse` output over the sampled keys — no (H*W x 10 960) matrix)
and the bilinear objective with its analytic translation gradient (isr_refine_objective) — the
reference builds both with torch autograd and a cv2.Rodrigues round trip per evaluation.  BFGS stays
scipy.optimize.minimize on the host, as in the reference (refine_poses(optimizer="device") runs a port of it on the device).  As there, only the translation is
optimised (the objective's rotation is a constant, pose_refine.py:73-76): R is returned unchanged.
`optimize_rotation=True` (off by default) is the evidently intended variant: the 6-vector is
(rotation vector, translation), the device returns d score / d R as well and the host chains it with the
Rodrigues Jacobian.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
from scipy.optimize import minimize

from . import ops
from ._capi import check, current_stream, lib, ptr, require_cuda
from .fields import KeyField
from .registration import _dev


INTERPOLATION = {"bilinear": 0, "nearest": 1, "bicubic": 2}     # F.grid_sample's modes -> ISR_INTERP_*


class RefineObjective:
    """score(t), grad(t) of pose_refine.py:70-91 for a fixed rotation, evaluated on the device."""

    def __init__(self, coord_obj: torch.Tensor, keys_masked: torch.Tensor, query_img: torch.Tensor,
                 denom_img: torch.Tensor, K_crop, R, interpolation: str = "bilinear"):
        if interpolation not in INTERPOLATION:
            raise ValueError(f"interpolation={interpolation!r}: F.grid_sample knows {sorted(INTERPOLATION)}")
        self.mode = INTERPOLATION[interpolation]
        self.dev = require_cuda(coord_obj, keys_masked, query_img, denom_img)
        self.X = coord_obj.to(torch.float32).contiguous()
        self.keys = keys_masked.to(torch.float32).contiguous()
        self.q = query_img.to(torch.float32).contiguous()
        self.den = denom_img.to(torch.float32).reshape(query_img.shape[0], query_img.shape[1]).contiguous()
        self.K = (ctypes.c_double * 9)(*np.asarray(K_crop, np.float64).reshape(9).tolist())
        self.R = np.asarray(R, np.float64).reshape(3, 3)
        self.out = torch.empty(13, dtype=torch.float64, device=self.dev)
        self.out_host = torch.empty(13, dtype=torch.float64).pin_memory()
        self.ws = ops.workspace(self.dev, 1 << 16, "refine_obj")
        self.n_launch = 0                 # device evaluations so far
        self._last = None                 # (pose bytes, full) -> outputs of the last evaluation

    def _eval(self, t, R=None, full=False):
        """One launch per distinct pose: BFGS asks for the value and then for the gradient at the same point
        (`fun` and `jac` are separate callables in the reference, pose_refine.py:93-101) — the kernel returns both."""
        Rm = self.R if R is None else np.asarray(R, np.float64).reshape(3, 3)
        Rt = np.concatenate([Rm, np.asarray(t, np.float64).reshape(3, 1)], axis=1).reshape(12)
        tag = (Rt.tobytes(), bool(full))
        if self._last is not None and self._last[0] == tag:
            return self._last[1]
        rt = (ctypes.c_double * 12)(*Rt.tolist())
        N, e = self.keys.shape
        fn = lib().isr_refine_objective_full if full else lib().isr_refine_objective
        with torch.cuda.device(self.dev):
            rc = fn(ptr(self.X), ptr(self.keys), N, e, ptr(self.q), ptr(self.den), self.q.shape[0], self.mode,
                    ctypes.cast(self.K, ctypes.c_void_p), ctypes.cast(rt, ctypes.c_void_p), ptr(self.out), ptr(self.ws),
                    self.ws.numel(), current_stream(self.dev))
            check(rc, "isr_refine_objective")
            self.out_host.copy_(self.out, non_blocking=True)
            torch.cuda.current_stream(self.dev).synchronize()
        self.n_launch += 1
        res = self.out_host.numpy()[: 13 if full else 4].copy()
        self._last = (tag, res)
        return res

    def with_rotation(self, pose, return_grad=False):
        """The 6-vector is (rotation vector, t): score, or its gradient (d/d rvec by the Rodrigues Jacobian)."""
        pose = np.asarray(pose, np.float64)
        R, dR = rodrigues(pose[:3])
        o = self._eval(pose[3:], R, full=True)
        if return_grad:
            return np.concatenate([np.einsum("jk,ijk->i", o[4:].reshape(3, 3), dR), o[1:4]])
        return float(o[0])

    def __call__(self, pose, return_grad=False):
        """pose: the reference's 6-vector (rvec ignored, t = pose[3:])."""
        o = self._eval(np.asarray(pose, np.float64)[3:])
        if return_grad:
            return np.concatenate([np.zeros(3), o[1:]])       # autograd leaves the unused rvec slots at 0
        return float(o[0])


def rodrigues(rvec):
    """cv2.Rodrigues(rvec) -> (R (3,3), dR (3,3,3) with dR[i] = d R / d rvec_i) in f64 (Gallego & Yezzi 2015:
    dR/dr_i = (r_i [r]x + [r x (I - R) e_i]x) R / |r|^2; [e_i]x at r = 0)."""
    r = np.asarray(rvec, np.float64).reshape(3)

    def skew(v):
        return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    th2 = float(r @ r)
    if th2 < 1e-24:
        return np.eye(3) + skew(r), np.stack([skew(e) for e in np.eye(3)])
    th = np.sqrt(th2)
    Kx = skew(r / th)
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    dR = np.stack([(r[i] * skew(r) + skew(np.cross(r, (np.eye(3) - R) @ np.eye(3)[i]))) @ R / th2 for i in range(3)])
    return R, dR


def denominator_image(query_img: torch.Tensor, keys_sampled: torch.Tensor) -> torch.Tensor:
    """pose_refine.py:56: logsumexp(query_img @ keys_sampled.T, -1) -> (H, W, 1): an lse-only call of K1."""
    H, W, e = query_img.shape
    lse = ops.corr_lse(query_img.reshape(H * W, e).to(torch.float32), keys_sampled.to(torch.float32))
    return lse.reshape(H, W, 1)


def refine_pose(R, t, query_img, renderer, obj_idx, K_crop, obj_, neural_radiance_field, keys_verts,
                interpolation='bilinear', n_samples_denom=10960, method='BFGS', *, generator=None,
                optimize_rotation=False):
    """pose_refine.py:21-104.  Returns (R, t (3,), result.fun).  optimize_rotation=True also refines R (returned
    as Rodrigues(result.x[:3])); the default keeps the reference's behaviour (R constant, returned unchanged)."""
    if interpolation not in INTERPOLATION:
        raise ValueError(f"interpolation={interpolation!r}: F.grid_sample knows {sorted(INTERPOLATION)}")
    query_img = _dev(query_img, torch.float32)
    h, w, _ = query_img.shape
    assert h == w
    dev = query_img.device
    t = np.asarray(t, np.float64).reshape(3)
    coord_img = renderer.render(obj_idx, K_crop, R, np.expand_dims(t, axis=1))
    coord_img = coord_img.cpu().numpy() if isinstance(coord_img, torch.Tensor) else np.asarray(coord_img)
    mask = coord_img[..., 3] == 1.
    coord_norm_masked = torch.from_numpy(np.ascontiguousarray(coord_img[..., :3][mask])).to(dev)
    coord_masked = coord_norm_masked * obj_.scale + torch.from_numpy(np.asarray(obj_.offset)).to(dev)
    coord_nerf = torch.from_numpy((coord_masked.cpu().numpy() * 1.8 / obj_.diameter).astype("float32")).to(dev)
    feat = neural_radiance_field.batched_customForward(coord_nerf).detach().clone()
    keys_masked = feat[..., :feat.shape[-1] - 1]                                   # drop the silhouette channel
    keys_verts = _dev(keys_verts, torch.float32)
    perm = torch.randperm(len(keys_verts), device=dev, generator=generator)[:n_samples_denom]
    denom_img = denominator_image(query_img, keys_verts[perm])
    obj = RefineObjective(coord_masked.float(), keys_masked.float(), query_img, denom_img, K_crop, R, interpolation)
    if optimize_rotation:
        from scipy.spatial.transform import Rotation
        rvec = Rotation.from_matrix(np.asarray(R, np.float64)).as_rotvec()
        pose = np.array([rvec[0], rvec[1], rvec[2], t[0], t[1], t[2]], dtype=np.float64)
        result = minimize(fun=obj.with_rotation, x0=pose, jac=lambda p: obj.with_rotation(p, return_grad=True), method=method)
        return rodrigues(result.x[:3])[0], result.x[3:], result.fun
    pose = np.array([0, 0, 0, t[0], t[1], t[2]], dtype=np.float64)
    result = minimize(fun=obj, x0=pose, jac=lambda p: obj(p, return_grad=True), method=method)
    return R, result.x[3:], result.fun


# ---------------------------------------------------------------------------------------------- a16 for a block of crops

class _Abort(BaseException):
    """Ends a lockstep worker whose siblings or caller failed (BaseException: scipy does not catch it)."""


def lockstep_minimize(x0s, batch_eval, method='BFGS', **minimize_kw):
    """One scipy.optimize.minimize per problem, each on a worker thread, their evaluations served in lockstep rounds.

    batch_eval(requests) gets [(problem, x), ...] — one pending point per live problem — and returns [(fun, jac), ...] in the
    same order; it is called on the calling thread only (the only thread that touches torch / HIP).  A worker's `fun` and `jac`
    post their point and block; when every live worker is blocked or finished the caller evaluates all pending points with one
    batch_eval call.  `fun` and `jac` at the point last evaluated for a problem share that evaluation (RefineObjective._eval).
    Every run sees only its own values, so problem k's result is that of minimize(fun_k, x0s[k], jac=jac_k, method=method,
    **minimize_kw).  A worker's exception (or batch_eval's) is re-raised here after every worker has ended.
    Returns (list of OptimizeResult, number of batch_eval calls)."""
    import threading

    n = len(x0s)
    cond = threading.Condition()     # the caller waits on it alone: notified only when the round is complete
    wake = [threading.Event() for _ in range(n)]     # one per worker: a served round wakes each worker once
    pending = {}                     # problem -> x posted and not yet served
    served = {}                      # problem -> (fun, jac) of its pending point
    state = {"live": n, "abort": False, "error": None}
    results = [None] * n

    def request(k, x):
        with cond:
            if state["abort"]:
                raise _Abort()
            pending[k] = x
            if len(pending) == state["live"]:
                cond.notify()
        wake[k].wait()
        wake[k].clear()
        with cond:
            if state["abort"]:
                raise _Abort()
            return served.pop(k)

    def worker(k):
        last = [None, None]          # x bytes, (fun, jac)

        def evaluate(x):
            x = np.array(x, dtype=np.float64)
            key = x.tobytes()
            if last[0] != key:
                last[1] = request(k, x)
                last[0] = key
            return last[1]

        try:
            results[k] = minimize(fun=lambda x: evaluate(x)[0], x0=np.asarray(x0s[k], np.float64),
                                  jac=lambda x: evaluate(x)[1], method=method, **minimize_kw)
        except _Abort:
            pass
        except BaseException as exc:          # noqa: BLE001 — handed to the caller
            with cond:
                if state["error"] is None:
                    state["error"] = exc
                state["abort"] = True
            for ev in wake:
                ev.set()
        finally:
            with cond:
                state["live"] -= 1
                if state["abort"] or len(pending) >= state["live"]:
                    cond.notify()

    threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(n)]
    for th in threads:
        th.start()
    rounds = 0
    try:
        while True:
            with cond:
                while not state["abort"] and state["live"] > 0 and len(pending) < state["live"]:
                    cond.wait()
                if state["abort"] or state["live"] == 0:
                    break
                reqs = sorted(pending.items())
                pending.clear()
            vals = batch_eval(reqs)
            rounds += 1
            if len(vals) != len(reqs):
                raise ValueError(f"batch_eval returned {len(vals)} results for {len(reqs)} requests")
            with cond:
                for (k, _), v in zip(reqs, vals):
                    served[k] = v
            for k, _ in reqs:
                wake[k].set()
    except BaseException:
        with cond:
            state["abort"] = True
        for ev in wake:
            ev.set()
        for th in threads:
            th.join()
        raise
    for th in threads:
        th.join()
    if state["error"] is not None:
        raise state["error"]
    return results, rounds


_BFGS_MESSAGES = {0: "Optimization terminated successfully.", 1: "Maximum number of iterations has been exceeded.",
                  2: "Desired error not necessarily achieved due to precision loss.",
                  3: "NaN result encountered."}


def bfgs_host(fun_and_grad, x0, gtol=1e-5, maxiter=None):
    """minimize(fun, x0, jac=..., method='BFGS', options={gtol, maxiter}) by the library's BFGS state machine run as host
    code — the code isr_refine_bfgs_batch runs on the device, one item per thread.  fun_and_grad(x) -> (f, g); it is
    called once per distinct point.  Returns an OptimizeResult (x, fun, nit, nfev, status, success, message) with
    n_wolfe2, the number of line searches that fell back from wolfe1 to wolfe2."""
    from scipy.optimize import OptimizeResult
    x0 = np.asarray(x0, np.float64).reshape(-1)
    n = x0.shape[0]
    maxiter = 200 * n if maxiter is None else int(maxiter)
    L = lib()
    state = ctypes.create_string_buffer(L.isr_bfgs_state_bytes())
    x = np.empty(n, np.float64)
    g = np.empty(n, np.float64)
    fun = ctypes.c_double()
    info = (ctypes.c_int32 * 5)()
    check(L.isr_bfgs_host_init(state, len(state), n, x0.ctypes.data_as(ctypes.c_void_p), float(gtol), maxiter,
                               x.ctypes.data_as(ctypes.c_void_p)), "isr_bfgs_host_init")
    while True:
        f, gr = fun_and_grad(x.copy())
        g[:] = np.asarray(gr, np.float64).reshape(n)
        check(L.isr_bfgs_host_step(state, float(f), g.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.byref(fun), info), "isr_bfgs_host_step")
        if info[0]:
            break
    status = int(info[1])
    return OptimizeResult(x=x.copy(), fun=fun.value, nit=int(info[2]), nfev=int(info[3]), status=status,
                          success=status == 0, message=_BFGS_MESSAGES[status], n_wolfe2=int(info[4]))


def refine_poses(Rs, ts, query_imgs, renderer, obj_idx, K_crops, obj_, neural_radiance_field, keys_verts,
                 interpolation='bilinear', n_samples_denom=10960, method='BFGS', *, seeds=None, optimize_rotation=False,
                 stats=None, optimizer="scipy", max_rounds=100_000):
    """refine_pose for a block of B crops of one object, the B BFGS runs in lockstep (lockstep_minimize): every round is one
    pinned H2D copy of the pending poses, ONE isr_refine_objective_batch launch for all of them, one D2H copy and one
    synchronise — instead of one launch + synchronise per image and evaluation.
    Rs (B,3,3), ts (B,3), query_imgs (B,res,res,e), K_crops one (3,3) or (B,3,3).  Image b's (R, t, fun) is bit for bit
    refine_pose(Rs[b], ts[b], query_imgs[b], ..., generator=torch.Generator(dev).manual_seed(seeds[b])) (seeds default
    range(B)): the same renderer / batched_customForward calls per image, the same key sample and denominator image, the same
    objective bits, the same scipy run.  A renderer with render_batch (render.ObjCoordRenderer) draws the block's images in
    one call and their visible coordinates are compacted on the device; any other renderer is called once per image as
    refine_pose calls it.  A fields.KeyField as neural_radiance_field evaluates the block's visible points in one call (its
    rows are independent, so the slices are the per-image bits); any other field is called once per image.
    Returns a list of B (R, t, fun).  stats (a dict, optional) receives rounds, n_eval (item evaluations per image) and
    launches.
    optimizer="device": the same renders, keys, key samples and denominator images, then ONE isr_refine_bfgs_batch call —
    scipy's BFGS ported to a per-item state machine that runs on the device (one objective launch and one step launch per
    round, the host reads the live count once per 8 rounds).  Each image's result equals bfgs_host driven by
    RefineObjective bit for bit, and scipy's to rounding.  BFGS over t only (method='BFGS', optimize_rotation=False);
    stats also receives nit and status (scipy's, or 4 when max_rounds ran out first)."""
    if optimizer not in ("scipy", "device"):
        raise ValueError(f"optimizer={optimizer!r}: 'scipy' or 'device'")
    if optimizer == "device" and (method != "BFGS" or optimize_rotation):
        raise ValueError("optimizer='device' runs BFGS over the translation only (method='BFGS', optimize_rotation=False)")
    if interpolation not in INTERPOLATION:
        raise ValueError(f"interpolation={interpolation!r}: F.grid_sample knows {sorted(INTERPOLATION)}")
    query_imgs = _dev(query_imgs, torch.float32)
    B = len(Rs)
    if query_imgs.ndim != 4 or query_imgs.shape[0] != B or len(ts) != B or query_imgs.shape[1] != query_imgs.shape[2]:
        raise ValueError(f"refine_poses: {B} rotations, {len(ts)} translations, query_imgs {tuple(query_imgs.shape)} "
                         "(B,res,res,e)")
    if B == 0:
        return []
    dev = query_imgs.device
    res, e = query_imgs.shape[1], query_imgs.shape[3]
    Ks = np.asarray(K_crops, np.float64)
    K_b = [K_crops] * B if Ks.ndim == 2 else [K_crops[b] for b in range(B)]     # the renderer gets what refine_pose would
    Ks = np.broadcast_to(Ks, (B, 3, 3)) if Ks.ndim == 2 else Ks.reshape(B, 3, 3)
    seeds = list(range(B)) if seeds is None else list(seeds)
    Rs_in = list(Rs)                                    # handed to the renderer and returned as given, as refine_pose does
    Rs = [np.asarray(R, np.float64).reshape(3, 3) for R in Rs_in]
    ts = [np.asarray(t, np.float64).reshape(3) for t in ts]
    # the renders first: an image with nothing visible fails before anything is launched
    Xs, keys = [], []
    block_field = isinstance(neural_radiance_field, KeyField)     # its rows are independent: the block's points in ONE call
    if hasattr(renderer, "render_batch"):
        # one call for the block's images; the visible coordinates never leave the device until the field's input is formed
        imgs = renderer.render_batch(obj_idx, Ks, Rs_in, ts).to(dev)
        mask = imgs[..., 3] == 1.
        counts = mask.reshape(B, -1).sum(1).cpu().numpy()
        if (counts == 0).any():
            raise ValueError(f"refine_poses: image {int(np.argmax(counts == 0))} renders no visible surface point at its start pose")
        ends = np.cumsum(counts)
        # row-major compaction, image after image: the order of coord_img[..., :3][mask]; then refine_pose's arithmetic,
        # element by element, on the whole block at once
        coord_norm_masked = imgs[..., :3][mask]
        coord_masked = coord_norm_masked * obj_.scale + torch.from_numpy(np.asarray(obj_.offset)).to(dev)
        coord_nerf = torch.from_numpy((coord_masked.cpu().numpy() * 1.8 / obj_.diameter).astype("float32")).to(dev)
        X_block = coord_masked.float()
        feat_block = neural_radiance_field.batched_customForward(coord_nerf) if block_field else None
        for b in range(B):
            lo, hi = int(ends[b] - counts[b]), int(ends[b])
            if block_field:
                feat = feat_block[lo:hi]
            else:
                feat = neural_radiance_field.batched_customForward(coord_nerf[lo:hi].clone()).detach().clone()
            Xs.append(X_block[lo:hi])
            keys.append(feat[..., :feat.shape[-1] - 1].float())
    else:
        renders = []
        for b in range(B):
            coord_img = renderer.render(obj_idx, K_b[b], Rs_in[b], np.expand_dims(ts[b], axis=1))
            coord_img = coord_img.cpu().numpy() if isinstance(coord_img, torch.Tensor) else np.asarray(coord_img)
            mask = coord_img[..., 3] == 1.
            if not mask.any():
                raise ValueError(f"refine_poses: image {b} renders no visible surface point at its start pose")
            renders.append((coord_img, mask))
        nerf_in = []
        for coord_img, mask in renders:                     # pose_refine.py:38-53, per image, as refine_pose does it
            coord_norm_masked = torch.from_numpy(np.ascontiguousarray(coord_img[..., :3][mask])).to(dev)
            coord_masked = coord_norm_masked * obj_.scale + torch.from_numpy(np.asarray(obj_.offset)).to(dev)
            coord_nerf = torch.from_numpy((coord_masked.cpu().numpy() * 1.8 / obj_.diameter).astype("float32")).to(dev)
            Xs.append(coord_masked.float())
            if block_field:
                nerf_in.append(coord_nerf)
                continue
            feat = neural_radiance_field.batched_customForward(coord_nerf).detach().clone()
            keys.append(feat[..., :feat.shape[-1] - 1].float())
        if block_field:
            feat_block = neural_radiance_field.batched_customForward(torch.cat(nerf_in))
            keys = [f[..., :f.shape[-1] - 1] for f in feat_block.split([x.shape[0] for x in nerf_in])]
    # the B lse-only denominator calls back to back (each image's own key sample: its generator), no host synchronise
    keys_verts = _dev(keys_verts, torch.float32)
    denoms = []
    for b in range(B):
        g = torch.Generator(device=dev).manual_seed(int(seeds[b]))
        perm = torch.randperm(len(keys_verts), device=dev, generator=g)[:n_samples_denom]
        denoms.append(denominator_image(query_imgs[b], keys_verts[perm]).reshape(res, res))
    # the visible sets, once per block
    counts = [x.shape[0] for x in Xs]
    offs = np.zeros(B + 1, np.int32)
    offs[1:] = np.cumsum(counts)
    X_all, keys_all = torch.cat(Xs).contiguous(), torch.cat(keys).contiguous()
    offs_dev = torch.from_numpy(offs).to(dev)
    q_all = query_imgs.contiguous()
    den_all = torch.stack(denoms).contiguous()
    K_dev = torch.from_numpy(np.ascontiguousarray(Ks.reshape(B, 9))).to(dev)
    mode = INTERPOLATION[interpolation]
    if optimizer == "device":
        R_dev = torch.from_numpy(np.ascontiguousarray(np.stack(Rs).reshape(B, 9))).to(dev)
        t_dev = torch.from_numpy(np.ascontiguousarray(np.stack(ts))).to(dev)
        item_dev = torch.arange(B, dtype=torch.int32, device=dev)
        r = ops.refine_bfgs_batch(X_all, keys_all, offs, q_all, den_all, K_dev, item_dev, R_dev, t_dev, mode,
                                  max_rounds=max_rounds, offs_dev=offs_dev)
        t_h, fun_h = r["t"].cpu().numpy(), r["fun"].cpu().numpy()
        nit, nfev, status = (r[k].cpu().numpy() for k in ("nit", "nfev", "status"))
        if stats is not None:
            stats.update(rounds=r["rounds"], launches=r["launches"], n_eval=nfev.tolist(), nit=nit.tolist(),
                         status=status.tolist())
        return [(Rs_in[b], t_h[b].copy(), float(fun_h[b])) for b in range(B)]
    nout = 13 if optimize_rotation else 4
    # one pinned staging buffer -> ONE H2D copy per round: [Rt (B,12) f64 | item_img (B,) i32]
    stage_h = torch.empty(B * 100, dtype=torch.uint8).pin_memory()
    stage_d = torch.empty(B * 100, dtype=torch.uint8, device=dev)
    Rt_h, item_h = stage_h[:B * 96].view(torch.float64).view(B, 12), stage_h[B * 96:].view(torch.int32)
    Rt_d, item_d = stage_d[:B * 96].view(torch.float64).view(B, 12), stage_d[B * 96:].view(torch.int32)
    out_d = torch.empty((B, nout), dtype=torch.float64, device=dev)
    out_h = torch.empty((B, nout), dtype=torch.float64).pin_memory()
    n_eval = [0] * B
    stream = torch.cuda.current_stream(dev)

    def batch_eval(reqs):
        n = len(reqs)
        jac_R = []
        Rt_np, item_np = Rt_h.numpy(), item_h.numpy()
        for i, (b, x) in enumerate(reqs):
            if optimize_rotation:
                R, dR = rodrigues(x[:3])
                jac_R.append(dR)
            else:
                R = Rs[b]
            Rt_np[i] = np.concatenate([R, np.asarray(x[3:], np.float64).reshape(3, 1)], axis=1).reshape(12)
            item_np[i] = b
            n_eval[b] += 1
        with torch.cuda.device(dev):
            stage_d.copy_(stage_h, non_blocking=True)
            ops.refine_objective_batch(X_all, keys_all, offs, q_all, den_all, K_dev, item_d, Rt_d, nout, mode,
                                       offs_dev=offs_dev, n_items=n, out=out_d)
            out_h[:n].copy_(out_d[:n], non_blocking=True)
            stream.synchronize()
        vals = []
        out_np = out_h.numpy()
        for i in range(n):
            o = out_np[i].copy()
            if optimize_rotation:                       # RefineObjective.with_rotation
                g = np.concatenate([np.einsum("jk,ijk->i", o[4:].reshape(3, 3), jac_R[i]), o[1:4]])
            else:                                       # RefineObjective.__call__
                g = np.concatenate([np.zeros(3), o[1:]])
            vals.append((float(o[0]), g))
        return vals

    if optimize_rotation:
        from scipy.spatial.transform import Rotation
        x0s = []
        for b in range(B):
            rvec = Rotation.from_matrix(Rs[b]).as_rotvec()
            x0s.append(np.array([rvec[0], rvec[1], rvec[2], ts[b][0], ts[b][1], ts[b][2]], dtype=np.float64))
    else:
        x0s = [np.array([0, 0, 0, t[0], t[1], t[2]], dtype=np.float64) for t in ts]
    results, rounds = lockstep_minimize(x0s, batch_eval, method=method)
    if stats is not None:
        stats.update(rounds=rounds, launches=rounds, n_eval=list(n_eval))
    if optimize_rotation:
        return [(rodrigues(r.x[:3])[0], r.x[3:], r.fun) for r in results]
    return [(Rs_in[b], r.x[3:], r.fun) for b, r in enumerate(results)]
