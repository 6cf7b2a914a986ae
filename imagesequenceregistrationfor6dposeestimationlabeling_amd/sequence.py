"""The per-sequence driver: what finalposes.py:105-238 / choosePose.py:154-309 (per-image
registration), verfication.py:61-108 (consecutive-pair Chamfer pick) and icp.py:37-126 (ICP +
final Chamfer) do, as one asynchronous pipeline per image on the HIP stream and one reduction per
sequence.  Everything between the encoder output and the pose stays on the device: the reference's
idx.cpu() / nidx.cpu() round trips (inference.py:273-290) are gone because the kept count M and
the RANSAC status live in device memory.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops, pose_est_surf, pose_refine, registration, shard


@dataclass
class SequenceModel:
    """First-sequence model as exported by genFeat.py:223-228 (vert1_scaled / feat1_scaled)."""
    keys: torch.Tensor   # (N, D) descriptors on the device, bf16 (MFMA bf16 path) or f32 (exact path)
    pts: torch.Tensor    # (N, 3) f32 surface points, mm
    log2_queries: bool = False   # bf16 queries carry a log2(e) prescale (ops.prescale_queries_log2)
    screened: bool = False       # with log2_queries: ISR_DTYPE_BF16_LOG2_SCREENED (K1 behind the FP6 screen; peaked softmaxes)


# True: the group routes (register_crops, register_block) let K1's epilogue form the first histogram of the top-80 % cut
# (isr_corr_argmax_digits -> isr_select_top_batch_digits): the same results, nine launches instead of ten and
# one read of logp less per group.  OFF by default: K1 is bound by its wave slots, and the counts — one device-scope integer
# atomic per wave and distinct digit, 770 000 per 32-image launch on ~20 addresses per image — hold the finishing waves' slots:
# 29.1 against 26.9 ms per launch alone, the step 5 % slower (profiles/r05_epilogue_histogram_ab.txt; bench.py --epilogue-digits).
EPILOGUE_DIGITS = False


@dataclass
class ImageResult:
    pose: torch.Tensor     # (3,4) f64 device [R|t]
    status: torch.Tensor   # (1,) i32 device
    n_inl: torch.Tensor    # (1,) i32 device
    inl_idx: torch.Tensor  # (P,) i32 device (first n_inl valid; indices into the kept set)
    keep: torch.Tensor     # (P,) i32 device (first M valid): nidx of inference.py:289
    M: torch.Tensor        # (1,) i32 device
    idx: torch.Tensor      # (P,) i32 device: idx1 of inference.py:273
    logp: torch.Tensor     # (P,) f32 device: in1[:,0]
    n_eval: torch.Tensor | None = None   # (1,) i32 device: hypotheses the staged RANSAC loop scored (sequential: that ran)


def register_image(model: SequenceModel, queries: torch.Tensor, pix_xy: torch.Tensor, cam,
                   itr: int = 500, reperr: float = 2.0, seed: int = 0, refine_iters: int = 10,
                   timing: list | None = None, confidence: float = 0.99, loop: str = "staged",
                   inliers: str = "refit", final: str = "refit") -> ImageResult:
    """inference.py:273-293 for one image, fully enqueued (no host synchronisation):
    getCors -> top-80 % filter -> correspondence assembly -> pnp(itr, reperr, P3P).  loop / inliers / final: ops.pnp_ransac's."""
    ops._loop_args(loop, inliers, None, final)
    if timing is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    idx, logp = ops.corr_argmax(queries, model.keys, log2_prescaled=model.log2_queries, screened=model.screened and model.log2_queries)
    if timing is not None:
        e1.record()
        timing.append((e0, e1))
    keep, M, _ = ops.select_top(logp)
    p3d, p2d = ops.gather_corr(idx, keep, M, model.pts, pix_xy)
    r = ops.pnp_ransac(p3d, p2d, cam, H=itr, reperr=reperr, seed=seed, refine_iters=refine_iters, M_dev=M,
                       confidence=confidence, loop=loop, inliers=inliers, final=final)
    return ImageResult(r.pose, r.status, r.n_inl, r.inl_idx, keep, M, idx, logp, r.n_eval)


def register_crop(model: SequenceModel, feat: torch.Tensor, mask: torch.Tensor, cam, c0: int = 0,
                  n_feat: int | None = None, down_sample: int = 3, itr: int = 500, reperr: float = 2.0,
                  seed: int = 0, refine_iters: int = 10, confidence: float = 0.99, loop: str = "staged",
                  inliers: str = "refit", final: str = "refit") -> tuple[ImageResult, torch.Tensor]:
    """inference.py:248-293 from the network output on: `feat` = imfeatsfull (1, H, W, C) or (H, W, C)
    channels-last on the device, `mask` = cropMask (H, W[, 3]) uint8 on the device, `cam` the cropped
    and down-sampled camera matrix (formats.crop_camera).  Sub-sampling, masking, the compaction of the
    masked descriptors into K1's operand layout and the pixel list run on the device
    (isr_prep_queries_batch); the number of masked pixels never visits the host.  Returns the ImageResult
    (arrays have the capacity ceil(H/ds) * ceil(W/ds); idx / logp rows past the count are padding) and
    the device count n_dev.  loop / inliers / final: ops.pnp_ransac's."""
    ops._loop_args(loop, inliers, None, final)
    D = model.keys.shape[1] if n_feat is None else n_feat
    if model.keys.dtype == torch.bfloat16:
        dtype = "bf16_log2" if model.log2_queries else "bf16"
    else:
        dtype = "f32"
    Q, pix, n_dev = ops.prep_queries(feat, mask, c0=c0, D=D, step=down_sample, dtype=dtype)
    keys = model.keys if model.keys.shape[1] == Q.shape[1] else ops._pad_cols(model.keys, Q.shape[1])
    idx, logp = ops.corr_argmax(Q, keys, log2_prescaled=model.log2_queries, screened=model.screened and model.log2_queries)
    keep, M, _ = ops.select_top(logp, n_dev=n_dev)
    p3d, p2d = ops.gather_corr(idx, keep, M, model.pts, pix)
    r = ops.pnp_ransac(p3d, p2d, cam, H=itr, reperr=reperr, seed=seed, refine_iters=refine_iters, M_dev=M,
                       confidence=confidence, loop=loop, inliers=inliers, final=final)
    return ImageResult(r.pose, r.status, r.n_inl, r.inl_idx, keep, M, idx, logp, r.n_eval), n_dev


def register_frame(model: SequenceModel, rgb, mask, camparams, encoder, n_feat: int = 12, down_sample: int = 3,
                   itr: int = 500, reperr: float = 2.0, seed: int = 0, refine_iters: int = 10, confidence: float = 0.99,
                   useMask: bool = True, loop: str = "staged", inliers: str = "refit", final: str = "refit"):
    """One iteration of the reference's per-image loop, inference.py:196-293, from the raw frame to the pose with
    everything but the descriptor network in this package: the crop front end on the device
    (registration.crop_inputs: mask box, crop affine + camera matrix, warp of image and mask, useMask blanking,
    normalize), `encoder` — the caller's network, `encoder_rgb` of inference.py:237: (1, 3, 224, 224) f32 ->
    (1, C, 224, 224) with the descriptor in channels [0, n_feat) — and then register_crop (sub-sampling, masking,
    getCors, top-80 % filter, pnp).  Returns (ImageResult, n_dev, camMat (3, 3))."""
    from . import registration
    ops._loop_args(loop, inliers, None, final)
    inputIM, cropMask, cam, _ = registration.crop_inputs(rgb, mask, camparams, useMask=useMask, down_sample=down_sample)
    with torch.no_grad():
        imfeatsfull = torch.movedim(encoder(inputIM), 1, 3)                       # inference.py:236-237
    res, n_dev = register_crop(model, imfeatsfull, cropMask[0], cam[0], n_feat=n_feat, down_sample=down_sample, itr=itr,
                               reperr=reperr, seed=seed, refine_iters=refine_iters, confidence=confidence, loop=loop,
                               inliers=inliers, final=final)
    return res, n_dev, cam[0]


def register_crops(model: SequenceModel, feats: torch.Tensor, masks: torch.Tensor, cams, c0: int = 0,
                   n_feat: int | None = None, down_sample: int = 3, itr: int = 500, reperr: float = 2.0,
                   seeds=None, refine_iters: int = 10, confidence: float = 0.99, group: int = 128,
                   n_streams: int = 1, loop: str = "staged", inliers: str = "refit",
                   final: str = "refit") -> tuple[list[ImageResult], torch.Tensor]:
    """The reference's per-image loop (inference.py:163, 248-293) from the network output on, BATCHED: `feats`
    (n, H, W, C) channels-last on the device, `masks` (n, H, W[, 3]) uint8 on the device, `cams` (n, 3, 3) the
    cropped, down-sampled camera matrices (formats.crop_camera).  Per `group` images: ONE isr_prep_queries_batch
    (three launches), ONE K1 launch on group * S capacity rows (S = ceil(H/ds) * ceil(W/ds); rows past an image's
    count are zero queries whose results nobody reads), ONE filter / assembly / RANSAC chain (register_group with
    the ragged counts).  At the reference's shape (75 x 75 crop, D = 12, N = 80 000) a single image is bound by
    ~45 dependent launches of a few microseconds of work each; a group shares them (0.6 launches per image at
    group = 64; 128-256 crops per group fill the chip best: K1's ~9 working workgroups per crop against 768 slots).  n_streams > 1 runs K1 of group g+1 on its own stream beside the chain of group g (slower at this
    shape, see below).  Every image's outputs are bit-identical to register_crop's.
    loop / inliers / final: ops.pnp_ransac's.  Returns (results, n_dev (n,) i32 on the device)."""
    ops._loop_args(loop, inliers, None, final)
    dev = model.keys.device
    n = feats.shape[0]
    D = model.keys.shape[1] if n_feat is None else n_feat
    if model.keys.dtype == torch.bfloat16:
        dtype = "bf16_log2" if model.log2_queries else "bf16"
    else:
        dtype = "f32"
    cams = np.asarray(cams, np.float64)
    cams = np.broadcast_to(cams, (n, 3, 3)) if cams.ndim == 2 else cams
    seeds = list(range(n)) if seeds is None else list(seeds)
    cur = torch.cuda.current_stream(dev)
    # n_streams <= 1 (the default here): everything on the caller's stream.  At this shape a K1 workgroup lives for
    # milliseconds (256 queries x 80 000 keys) and fills its CU's registers; a chain of ~50 small DEPENDENT launches
    # on a side stream then waits for a K1 workgroup to retire before each of its kernels can start (measured:
    # 207 us per gn_accumulate launch instead of ~8) and the chain, not K1, bounds the group.  In sequence the chain
    # costs ~0.4 ms per group behind a ~3 ms K1.  (bench.py's 640 x 480 shape is the opposite case: K1 is 30 ms
    # per launch and the chain hides beside it — sequence.register_block keeps its side streams.)
    serial = n_streams <= 1
    pool = [cur, cur] if serial else _stream_pool(dev, max(n_streams, 2))
    if not serial:
        for s in pool:
            s.wait_stream(cur)
    k1_stream, side = pool[0], pool[1:]
    out, counts, keys = [], [], None
    for gi, g0 in enumerate(range(0, n, group)):
        g1 = min(n, g0 + group)
        B = g1 - g0
        with torch.cuda.stream(k1_stream):
            Q, pix, n_dev = ops.prep_queries_batch(feats[g0:g1], masks[g0:g1], c0=c0, D=D, step=down_sample, dtype=dtype)
            if keys is None:
                keys = model.keys if model.keys.shape[1] == Q.shape[2] else ops._pad_cols(model.keys, Q.shape[2])
            S = Q.shape[1]
            # (the cut's first histogram is formed in K1's epilogue, of each crop's n_dev live rows: SURVEY 8(f)-2)
            if EPILOGUE_DIGITS:
                idx_g, logp_g, hist_g = ops.corr_argmax(Q.view(B * S, -1), keys, log2_prescaled=model.log2_queries,
                                                        screened=model.screened and model.log2_queries, rows_per_image=S, n_rows=n_dev)
            else:
                idx_g, logp_g = ops.corr_argmax(Q.view(B * S, -1), keys, log2_prescaled=model.log2_queries,
                                                screened=model.screened and model.log2_queries)
                hist_g = None
            if not serial:
                done = torch.cuda.Event()
                done.record(k1_stream)
        s = side[gi % len(side)]
        if not serial:
            s.wait_event(done)
            for t in (idx_g, logp_g, hist_g, pix, n_dev):
                if t is not None:
                    t.record_stream(s)
        with torch.cuda.stream(s):
            keep, M, _ = ops.select_top_batch(logp_g.view(B, S), n_dev=n_dev, digit_hist=hist_g)
            p3d, p2d = ops.gather_corr_batch(idx_g.view(B, S), keep, M, model.pts, pix)
            r = ops.pnp_ransac_batch(p3d, p2d, cams[g0:g1], M, H=itr, reperr=reperr, seeds=seeds[g0:g1],
                                     refine_iters=refine_iters, confidence=confidence, loop=loop, inliers=inliers, final=final)
        iv, lv = idx_g.view(B, S), logp_g.view(B, S)
        out += [ImageResult(r.pose[b], r.status[b:b + 1], r.n_inl[b:b + 1], r.inl_idx[b], keep[b], M[b:b + 1], iv[b], lv[b],
                            r.n_eval[b:b + 1]) for b in range(B)]
        counts.append(n_dev)
    if not serial:
        for s in pool:
            cur.wait_stream(s)
        _publish(out, cur)
        for n_dev in counts:              # allocated on k1_stream, read by the cat below on the caller's stream
            n_dev.record_stream(cur)
    n_all = torch.cat(counts)
    return out, n_all


def register_frames(model: SequenceModel, rgbs, masks, camparams, encoder, n_feat: int = 12, down_sample: int = 3,
                    itr: int = 500, reperr: float = 2.0, seeds=None, refine_iters: int = 10, confidence: float = 0.99,
                    useMask: bool = True, group: int = 128, loop: str = "staged", inliers: str = "refit", final: str = "refit"):
    """The reference's per-image loop, inference.py:163-293, for a block of frames: the crop front end of every
    frame on the device in two launches (registration.crop_inputs: mask boxes, crop affines + camera matrices,
    warps, useMask blanking, normalize), ONE call of `encoder` on the (n, 3, 224, 224) batch (the caller's network,
    `encoder_rgb` of inference.py:237), then register_crops.  Returns (results, n_dev (n,), camMat (n, 3, 3))."""
    ops._loop_args(loop, inliers, None, final)
    inputIM, cropMask, cam, _ = registration.crop_inputs(rgbs, masks, camparams, useMask=useMask, down_sample=down_sample)
    with torch.no_grad():
        imfeatsfull = torch.movedim(encoder(inputIM), 1, 3)                       # inference.py:236-237
    res, n_dev = register_crops(model, imfeatsfull, cropMask, cam, n_feat=n_feat, down_sample=down_sample, itr=itr,
                                reperr=reperr, seeds=seeds, refine_iters=refine_iters, confidence=confidence, group=group,
                                loop=loop, inliers=inliers, final=final)
    return res, n_dev, cam


def _publish(results: list[ImageResult], consumer: torch.cuda.Stream) -> None:
    """The tensors of `results` were allocated on side streams and are about to be read on `consumer`
    (which has been made to wait for those streams).  Tell the caching allocator: without
    record_stream a dropped result's block goes back to its side stream's pool at once, and the next
    step's allocations there may overwrite it while `consumer` is still reading."""
    for r in results:
        for t in (r.pose, r.status, r.n_inl, r.inl_idx, r.keep, r.M, r.idx, r.logp, r.n_eval):
            if t is not None:
                t.record_stream(consumer)


_streams: dict[tuple, list] = {}
_closed: dict[tuple, torch.cuda.Event] = {}       # (device, workspace tag) -> the event behind the last close on that workspace

# register_block: a group's K1 call is OPENED on the K1 stream (key norms + the chip-filling kernel) and CLOSED on the group's
# side stream (fallback, finalize, recheck, merge: ~170 us of small launches at low occupancy, ahead of the cut that reads their
# outputs), so that the next group's chip-filling kernel follows this one's directly: on one stream the closing kernels and the
# next call's key-norm kernel stood between them (K1's duty cycle 0.977, profiles/r05_side_work_budget.txt).  Two workspaces
# alternate; an opening waits for the close that last used its workspace.  The chip-filling kernels stay one behind the other on
# one stream (their durations mean what they say).  False: one isr_corr_argmax call per group.  Same results either way.
K1_SPLIT_CLOSE = True


def _stream_pool(dev: torch.device, n: int) -> list:
    key = (dev.index, n)
    if key not in _streams:
        # stream 0 carries K1; the side streams carry the per-image chains of small dependent launches
        # and get the higher priority: they need a few CUs for microseconds, and every microsecond
        # they wait for a slot is serial latency (measured: +2 % images/s, K1-high: -4 %)
        _streams[key] = [torch.cuda.Stream(device=dev, priority=0 if i == 0 else -1) for i in range(n)]
    return _streams[key]


def register_images(model: SequenceModel, images, cam, itr: int = 500, reperr: float = 2.0,
                    seed0: int = 0, refine_iters: int = 10, n_streams: int = 3,
                    confidence: float = 0.99, loop: str = "staged", inliers: str = "refit",
                    final: str = "refit") -> list[ImageResult]:
    """Register a block of images with the stages pipelined over HIP streams.

    Stream 0 runs nothing but K1 (getCors) back to back — the only kernel that fills the chip;
    image j's filter + assembly + RANSAC chain (a dozen small dependent launches) waits on K1(j)'s
    event and runs on side stream 1 + j % (n_streams - 1), beside K1(j+1) and inside K1's launch
    tail (a 640x480 image is 1.17 rounds of resident workgroups).  Events recorded around K1 on
    stream 0 therefore bracket the kernel alone.  `images` is a sequence of (queries, pix_xy);
    `cam` one 3x3 or one per image.  The caller's current stream waits for every stream before
    this returns; there is no host synchronisation.  loop / inliers / final: ops.pnp_ransac's."""
    ops._loop_args(loop, inliers, None, final)
    dev = model.keys.device
    cur = torch.cuda.current_stream(dev)
    cam_of = (lambda j: cam) if np.ndim(cam) == 2 else (lambda j: cam[j])
    if n_streams <= 1:
        return [register_image(model, q, pix, cam_of(j), itr, reperr, seed0 + j, refine_iters, confidence=confidence,
                               loop=loop, inliers=inliers, final=final)
                for j, (q, pix) in enumerate(images)]
    pool = _stream_pool(dev, n_streams)
    for s in pool:
        s.wait_stream(cur)
    k1_stream, side = pool[0], pool[1:]
    out = []
    for j, (q, pix) in enumerate(images):
        with torch.cuda.stream(k1_stream):
            idx, logp = ops.corr_argmax(q, model.keys, log2_prescaled=model.log2_queries, screened=model.screened and model.log2_queries)
            done = torch.cuda.Event()
            done.record(k1_stream)
        s = side[j % len(side)]
        s.wait_event(done)
        idx.record_stream(s)
        logp.record_stream(s)
        with torch.cuda.stream(s):
            keep, M, _ = ops.select_top(logp)
            p3d, p2d = ops.gather_corr(idx, keep, M, model.pts, pix)
            r = ops.pnp_ransac(p3d, p2d, cam_of(j), H=itr, reperr=reperr, seed=seed0 + j,
                               refine_iters=refine_iters, M_dev=M, confidence=confidence, loop=loop, inliers=inliers, final=final)
        out.append(ImageResult(r.pose, r.status, r.n_inl, r.inl_idx, keep, M, idx, logp, r.n_eval))
    for s in pool:
        cur.wait_stream(s)
    _publish(out, cur)
    return out


def register_group(model: SequenceModel, idx_g: torch.Tensor, logp_g: torch.Tensor, pix_xy: torch.Tensor, cams,
                   itr: int, reperr: float, seeds, refine_iters: int, confidence: float = 0.99,
                   digit_hist: torch.Tensor | None = None, loop: str = "staged", inliers: str = "refit",
                   final: str = "refit") -> list[ImageResult]:
    """inference.py:282-293 for a GROUP of images whose K1 results are idx_g / logp_g (B, P): the
    top-80 % filter, the correspondence assembly and pnp() run as ONE chain of launches with the
    image on blockIdx.z (isr_select_top_batch, isr_gather_corr_batch, isr_pnp_ransac_batch) — the
    same kernels as the per-image calls, so every image's outputs are bit-identical to
    register_image's.  pix_xy (P, 2) shared or (B, P, 2); cams one 3x3 or (B, 3, 3).  digit_hist (B, 2048): the cut's first
    histogram when K1 formed it (ops.corr_argmax(..., rows_per_image=P)).  loop / inliers / final: ops.pnp_ransac's."""
    ops._loop_args(loop, inliers, None, final)
    B = idx_g.shape[0]
    keep, M, _ = ops.select_top_batch(logp_g, digit_hist=digit_hist)
    p3d, p2d = ops.gather_corr_batch(idx_g, keep, M, model.pts, pix_xy)
    r = ops.pnp_ransac_batch(p3d, p2d, cams, M, H=itr, reperr=reperr, seeds=seeds, refine_iters=refine_iters,
                             confidence=confidence, loop=loop, inliers=inliers, final=final)
    return [ImageResult(r.pose[b], r.status[b:b + 1], r.n_inl[b:b + 1], r.inl_idx[b], keep[b], M[b:b + 1], idx_g[b], logp_g[b],
                        r.n_eval[b:b + 1])
            for b in range(B)]


def register_block(model: SequenceModel, queries: torch.Tensor, pix_xy: torch.Tensor, cam, itr: int = 500,
                   reperr: float = 2.0, seed0: int = 0, refine_iters: int = 10, n_streams: int = 3,
                   group: int = 8, confidence: float = 0.99, loop: str = "staged", inliers: str = "refit",
                   final: str = "refit") -> list[ImageResult]:
    """register_images for a block held as ONE tensor: queries (n, P, D), pix_xy (n, P, 2) or (P, 2).
    K1 runs once per `group` images on (group * P) query rows — K1's result for a query does not
    depend on the launch it rides in, so this only changes the launch shape: a 640x480 image alone is
    1.17 rounds of resident workgroups, sixteen together are 18.8, and the launch tail shrinks from
    ~20 % to ~2 % of K1's time.  The group's filter / assembly / RANSAC chain (register_group: ~30
    launches for the whole group instead of ~35 per image) runs on a side stream beside the next K1
    launch; groups alternate between the side streams.  loop / inliers / final: ops.pnp_ransac's."""
    ops._loop_args(loop, inliers, None, final)
    dev = model.keys.device
    n, P = queries.shape[0], queries.shape[1]
    cur = torch.cuda.current_stream(dev)
    cams = np.asarray(cam, np.float64)
    cams = np.broadcast_to(cams, (n, 3, 3)) if cams.ndim == 2 else cams
    pool = _stream_pool(dev, max(n_streams, 2))
    for s in pool:
        s.wait_stream(cur)
    k1_stream, side = pool[0], pool[1:]
    kw = dict(log2_prescaled=model.log2_queries, screened=model.screened and model.log2_queries)
    if EPILOGUE_DIGITS:
        kw["rows_per_image"] = P
    out = []
    for gi, g0 in enumerate(range(0, n, group)):
        g1 = min(n, g0 + group)
        rows = queries[g0:g1].reshape((g1 - g0) * P, -1)
        with torch.cuda.stream(k1_stream):
            if K1_SPLIT_CLOSE:
                tag = f"corr{gi & 1}"
                prev = _closed.get((dev.index, tag))
                if prev is not None:
                    k1_stream.wait_event(prev)             # the workspace's last close (two groups ago: long finished)
                call = ops.corr_argmax_open(rows, model.keys, ws_tag=tag, **kw)
                res = call.outputs()
            else:
                res = ops.corr_argmax(rows, model.keys, **kw)
            done = torch.cuda.Event()
            done.record(k1_stream)
        s = side[gi % len(side)]
        s.wait_event(done)
        for t in res:
            t.record_stream(s)
        with torch.cuda.stream(s):
            if K1_SPLIT_CLOSE:
                ops.corr_argmax_close(call)
                closed = torch.cuda.Event()
                closed.record(s)
                _closed[(dev.index, tag)] = closed
            idx_g, logp_g = res[0], res[1]
            out += register_group(model, idx_g.view(g1 - g0, P), logp_g.view(g1 - g0, P),
                                  pix_xy if pix_xy.ndim == 2 else pix_xy[g0:g1], cams[g0:g1], itr, reperr,
                                  [seed0 + j for j in range(g0, g1)], refine_iters, confidence,
                                  digit_hist=res[2] if EPILOGUE_DIGITS else None, loop=loop, inliers=inliers, final=final)
    for s in pool:
        cur.wait_stream(s)
    _publish(out, cur)
    return out


def stack_poses(results: list[ImageResult]) -> tuple[torch.Tensor, torch.Tensor]:
    """(n,12) f64 poses and (n,) status, still on the device."""
    return (torch.stack([r.pose.reshape(12) for r in results]),
            torch.cat([r.status for r in results]))


def acceptance_counts(model_verts, surface_pts, R_gt, t_gt, poses: torch.Tensor, status: torch.Tensor, diameter: float,
                      dataset: str = "tless", names=None) -> dict:
    """The per-image acceptance bookkeeping of inference.py:300-320 for a whole block of registered images in two
    launches instead of two KD-tree builds per image:
        final_error  = ADDS(modelVerts, gtR, gtT, R2, T2)            (dataset == "tless";  ADD otherwise)
        final_errorR = ADDS(modelVerts, gtR, 0, R2, 0)               (rotation only)
        workCT += final_error < 0.1 * diameter;  rotWorkCT += final_errorR < 0.1 * diameter
        correct_predicted_ids.append(name)  for accepted images      (-> correctly_predicted_list.txt, :369-374)
    poses (n, 12) [R|t] f64 and status (n,) on the device (sequence.stack_poses).  An image whose pnp failed (status
    0; the reference's `(1, 1, 1)` sentinel would raise inside ADDS there) is never accepted: its errors are inf.
    Returns {final_error (n,), final_errorR (n,), work (n,) bool, rot_work (n,) bool, workCT, rotWorkCT,
    correct_predicted_ids}."""
    v = registration._dev(model_verts, torch.float32)
    n = poses.shape[0]
    Tp = poses.reshape(n, 3, 4).to(torch.float64)
    Tg = torch.cat([registration._dev(R_gt, torch.float64).reshape(n, 3, 3),
                    registration._dev(t_gt, torch.float64).reshape(n, 3, 1)], dim=2)
    Tp0, Tg0 = Tp.clone(), Tg.clone()
    Tp0[:, :, 3] = 0.0
    Tg0[:, :, 3] = 0.0
    if dataset == "tless":
        sp = registration._dev(surface_pts, torch.float32)
        # queries = GT-pose CAD vertices, targets = predicted-pose surface points (inference.py:118-120)
        err = ops.nn_batched(v, sp, Tg.reshape(n, 12), Tp.reshape(n, 12)).sum_d / v.shape[0]
        errR = ops.nn_batched(v, sp, Tg0.reshape(n, 12), Tp0.reshape(n, 12)).sum_d / v.shape[0]
    else:
        err = ops.add_metric(v, Tg.reshape(n, 12), Tp.reshape(n, 12))
        errR = ops.add_metric(v, Tg0.reshape(n, 12), Tp0.reshape(n, 12))
    ok = status.reshape(n) != 0
    inf = torch.full_like(err, float("inf"))
    err, errR = torch.where(ok, err, inf), torch.where(ok, errR, inf)
    host = torch.stack([err, errR]).cpu().numpy()           # one copy
    work, rot = host[0] < 0.1 * diameter, host[1] < 0.1 * diameter
    ids = [names[i] if names is not None else i for i in np.nonzero(work)[0]]
    return dict(final_error=host[0], final_errorR=host[1], work=work, rot_work=rot, workCT=int(work.sum()),
                rotWorkCT=int(rot.sum()), correct_predicted_ids=ids)


def estimate_and_refine(mask_lgts, query_imgs, obj_pts, obj_normals, obj_keys, obj_diameter, Ks, renderer, obj_idx, obj_,
                        neural_radiance_field, keys_verts, model_verts, R_gt, t_gt, *, seeds=None, refine_seeds=None,
                        estimate_kw=None, refine_kw=None) -> dict:
    """The useSurfEval branch of inference.py:324-366 for a block of B crops of one object:
        R, t, pose_scores, mask_scores, ... = estimate_pose(mask_lgts[b], query_imgs[b], ...)     (estimate_poses: one block)
        if len(mask_scores) > 0:
            bestId = torch.argsort(pose_scores)[-1];  R2, T2 = R[bestId], t[bestId]
            finADD  = ADD(modelVerts, gtR, gtT, R2, T2)
            _, t_ref, fun = refine_pose(R2, T2, query_imgs[b], ...)                                 (refine_poses: lockstep)
            refADD  = ADD(modelVerts, gtR, gtT, R2, t_ref)        (R2: the branch measures the refined translation only)
            finADDR = ADD(modelVerts, gtR, 0, R2, 0)
            refCT += refADD < 0.1 d;  workCT += finADD < 0.1 d;  rotWorkCT += finADDR < 0.1 d
    ADD on every dataset (the branch never uses ADD-S).  An image with no mask score is skipped, as there: never refined, never
    counted, refined[b] False and its per-image values NaN.  Image b uses estimate seed seeds[b] and refine seed refine_seeds[b]
    (both default b: refine_pose's key sample is torch.Generator(dev).manual_seed(refine_seeds[b])).  The three ADDs are three
    batched add_metric launches and one copy to the host.  Ks one (3,3) or (B,3,3); R_gt (B,3,3), t_gt (B,3).
    Returns {refined (B,) bool, R2 (B,3,3), T2 (B,3) f32, t_ref (B,3), fun (B,), finADD, refADD, finADDR (B,) f64,
    workCT, refCT, rotWorkCT}."""
    mask_lgts, query_imgs = registration._dev(mask_lgts, torch.float32), registration._dev(query_imgs, torch.float32)
    B = mask_lgts.shape[0]
    R_gt = np.asarray(R_gt, np.float64).reshape(-1, 3, 3) if np.size(R_gt) else np.zeros((0, 3, 3))
    t_gt = np.asarray(t_gt, np.float64).reshape(-1, 3) if np.size(t_gt) else np.zeros((0, 3))
    Ka = np.asarray(Ks, np.float64)
    if (mask_lgts.ndim != 3 or query_imgs.ndim != 4 or query_imgs.shape[0] != B or mask_lgts.shape[1:] != query_imgs.shape[1:3]
            or R_gt.shape[0] != B or t_gt.shape[0] != B or not (Ka.shape == (3, 3) or Ka.shape == (B, 3, 3))):
        raise ValueError(f"estimate_and_refine: mask_lgts {tuple(mask_lgts.shape)} query_imgs {tuple(query_imgs.shape)} "
                         f"R_gt {R_gt.shape} t_gt {t_gt.shape} Ks {Ka.shape}: (B,r,r) (B,r,r,e) (B,3,3) (B,3) (3,3)|(B,3,3)")
    seeds = list(range(B)) if seeds is None else list(seeds)
    refine_seeds = list(range(B)) if refine_seeds is None else list(refine_seeds)
    nan = np.full(B, np.nan)
    out = dict(refined=np.zeros(B, bool), R2=np.full((B, 3, 3), np.nan, np.float32), T2=np.full((B, 3), np.nan, np.float32),
               t_ref=np.full((B, 3), np.nan), fun=nan.copy(), finADD=nan.copy(), refADD=nan.copy(), finADDR=nan.copy(),
               workCT=0, refCT=0, rotWorkCT=0)
    if B == 0:
        return out
    est = pose_est_surf.estimate_poses(mask_lgts, query_imgs, obj_pts, obj_normals, obj_keys, obj_diameter, Ka, seeds=seeds,
                                       **(estimate_kw or {}))
    kept = [b for b in range(B) if len(est[b][3]) > 0]
    if not kept:
        return out
    best = [torch.argsort(est[b][2])[-1] for b in kept]
    Rt2 = torch.stack([torch.cat([est[b][0][i], est[b][1][i][:, None]], dim=1) for b, i in zip(kept, best)]).cpu().numpy()
    R2, T2 = Rt2[:, :, :3], Rt2[:, :, 3]                 # f32, the values of R[bestId].cpu().numpy(), t[bestId].cpu().numpy()
    refined = pose_refine.refine_poses([R2[i] for i in range(len(kept))], [T2[i] for i in range(len(kept))],
                                       query_imgs[kept], renderer, obj_idx, Ka if Ka.ndim == 2 else Ka[kept], obj_,
                                       neural_radiance_field, keys_verts, seeds=[refine_seeds[b] for b in kept],
                                       **(refine_kw or {}))
    t_ref = np.stack([np.asarray(r[1], np.float64).reshape(3) for r in refined])
    z = np.zeros(3)
    T_gt = registration._dev(np.stack([registration._pose12(R_gt[b], t_gt[b]) for b in kept]))
    T_gt0 = registration._dev(np.stack([registration._pose12(R_gt[b], z) for b in kept]))
    T_fin = registration._dev(np.stack([registration._pose12(R2[i], T2[i]) for i in range(len(kept))]))
    T_ref = registration._dev(np.stack([registration._pose12(R2[i], t_ref[i]) for i in range(len(kept))]))
    T_fin0 = registration._dev(np.stack([registration._pose12(R2[i], z) for i in range(len(kept))]))
    v = registration._dev(model_verts, torch.float32)
    adds = torch.stack([ops.add_metric(v, T_gt, T_fin), ops.add_metric(v, T_gt, T_ref),
                        ops.add_metric(v, T_gt0, T_fin0)]).cpu().numpy()          # one copy
    d = 0.1 * obj_diameter
    out["refined"][kept] = True
    out["R2"][kept], out["T2"][kept], out["t_ref"][kept] = R2, T2, t_ref
    out["fun"][kept] = [float(r[2]) for r in refined]
    out["finADD"][kept], out["refADD"][kept], out["finADDR"][kept] = adds[0], adds[1], adds[2]
    out.update(workCT=int((adds[0] < d).sum()), refCT=int((adds[1] < d).sum()), rotWorkCT=int((adds[2] < d).sum()))
    return out


def _orthonormal(R, tol=1e-9) -> bool:
    """R2 inv(R1) = R2 R1^T exactly when R1 is orthonormal (then np.linalg.inv and the transpose agree
    to rounding); scene_gt rotations with few printed digits fall back to the general inverse."""
    return bool(np.all(np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)) < tol))


def pick_by_chamfer(pc1: torch.Tensor, poses_all: torch.Tensor, R_gt_all: np.ndarray, t_gt_all: np.ndarray,
                    n_total: int) -> tuple[int, float]:
    """verfication.py:61-108 sharded: this rank evaluates the consecutive pairs it owns, then ONE
    all-reduce(MIN) over the (n - 1)-entry f64 table (shard.allreduce_min_table) hands every rank the whole
    `chamferdis` list, and min / list.index(min) — the first minimum, in f64 — is taken on every rank
    identically.  poses_all (n,12) predicted poses of ALL images (after the all-gather), R_gt_all/t_gt_all
    the GT poses from scene_gt.json.  Returns (index, value)."""
    idx, val, _ = pick_by_chamfer_table(pc1, poses_all, R_gt_all, t_gt_all, n_total)
    return idx, val


def chamfer_pairs_owned(pc1: torch.Tensor, poses_all: torch.Tensor, R_gt_all: np.ndarray, t_gt_all: np.ndarray,
                        lo: int, hi: int) -> torch.Tensor:
    """The device part of the sharded pick: the Chamfer values of the consecutive pairs (i, i+1), i in [lo, hi)
    (verfication.py:70-102) as a (hi - lo,) f64 device tensor.  A pair's value is a function of the two images'
    poses only, whichever block it is evaluated in."""
    if hi <= lo:
        return torch.empty(0, dtype=torch.float64, device=pc1.device)
    Rp = poses_all.reshape(-1, 3, 4)[lo:hi + 1, :, :3].cpu().numpy()
    # rotation block of [R2|T2] inv([R1|T1]) (verfication.py:9-19) for every owned pair at once
    Rg = np.asarray(R_gt_all, np.float64)
    Rrel = np.einsum("nij,nkj->nik", Rg[lo + 1:hi + 1], Rg[lo:hi]) if _orthonormal(Rg[lo:hi]) else np.stack(
        [registration.calculate_relative_pose(R_gt_all[i], t_gt_all[i], R_gt_all[i + 1], t_gt_all[i + 1])[0]
         for i in range(lo, hi)])
    return registration.chamfer_pairs(pc1, Rp, Rrel)


def pick_by_chamfer_table(pc1: torch.Tensor, poses_all: torch.Tensor, R_gt_all: np.ndarray, t_gt_all: np.ndarray,
                          n_total: int) -> tuple[int, float, np.ndarray]:
    """pick_by_chamfer, also returning the full chamferdis table (n - 1,) f64 as a NumPy array."""
    rank, size = shard.world()
    lo, hi = shard.owned_pairs(n_total, rank, size)
    ch = chamfer_pairs_owned(pc1, poses_all, R_gt_all, t_gt_all, lo, hi)
    table = shard.allreduce_min_table(ch, lo, n_total - 1).cpu().numpy()
    idx, val = shard.first_min(table)
    return idx, val, table


_field_cache: dict = {}


def cloud_key(pts: torch.Tensor) -> tuple:
    """(hash1, hash2, shape, dtype, device index) of a cloud's bytes: see surface_field."""
    flat = pts.detach().contiguous().view(-1)
    bits = flat.view(torch.int32 if flat.element_size() == 4 else torch.int64).to(torch.int64)
    i = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64)
    h1 = (bits * (2 * i + 1)).sum()                                    # int64 arithmetic wraps: sums modulo 2^64
    h2 = ((bits ^ (bits >> 15)) * (i * 0x9E3779B1 + 0x7F4A7C15 | 1)).sum()
    h = torch.stack([h1, h2]).cpu().numpy()
    return (int(h[0]), int(h[1]), tuple(pts.shape), str(pts.dtype), pts.device.index)


def surface_field(surface_pts: torch.Tensor, cells: int = 128) -> "ops.DistField":
    """The distance field of a surface cloud for vote_rows' bounds, built once per cloud."""
    # keyed by CONTENT (one small read-back): an address can be handed to another cloud of the same shape.  The key is a pair of
    # position-weighted wrapping int64 sums over the coordinates' BIT patterns (element i weighted by an odd multiplier that
    # depends on i), so a cloud with permuted axes, swapped rows or one changed coordinate gets another key (round 4 keyed on
    # two f64 sums that a within-row permutation left unchanged).
    key = cloud_key(surface_pts) + (cells,)
    fld = _field_cache.get(key)
    if fld is None:
        if len(_field_cache) > 4:
            _field_cache.clear()
        fld = _field_cache[key] = ops.dist_field(surface_pts, cells=cells)
    return fld


VOTE_SLACK_MM = 1e-3      # an item within this of the threshold is always evaluated exactly (f32 coordinates, field rounding)


def vote_rows(model_verts, surface_pts, R_gt, t_gt, R_pred, t_pred, diameter, lo: int, hi: int, chunk: int = 4096,
              bounds: bool | None = None, stats: dict | None = None):
    """The device part of the row-sharded vote (choosePose.py:98-107, 121-138): rows [lo, hi) of
        error[i][j] = ADDS(modelVerts, gt_rel[i][j], pred_rel[i][j]) < 0.1 * diameter
    Returns (error rows (hi - lo, n) bool device tensor, their int32 row sums (hi - lo, 1)).
    The vote needs the DECISION, not the ADD-S value.  bounds (default: on from 1 024 items): every item first gets a
    rigorous lower and upper bound of its ADD-S from a distance field of the surface cloud (ops.adds_bounds: one gather per
    vertex); only items whose bounds straddle 0.1 * diameter (+- VOTE_SLACK_MM) go through the nearest-neighbour search —
    the booleans are those of evaluating every item (tested).  stats (optional dict) receives the counts."""
    n = len(R_gt)
    v = registration._dev(model_verts, torch.float32)
    sp = registration._dev(surface_pts, torch.float32)
    Rg, tg = registration._dev(R_gt, torch.float64), registration._dev(t_gt, torch.float64)     # arrays or tensors
    Rp, tp = registration._dev(R_pred, torch.float64), registration._dev(t_pred, torch.float64)
    gt_rel = ops.rel_pose_table(Rg, tg, 0, lo, hi).reshape(-1, 12)        # (rows * n, 12) f64, [R_i^T R_j | t_j - t_i]
    pr_rel = ops.rel_pose_table(Rp, tp, 0, lo, hi).reshape(-1, 12)
    items = (hi - lo) * n
    thr = 0.1 * float(diameter)
    V = v.shape[0]

    def exact(sel_g, sel_p):
        parts = [ops.nn_batched(v, sp, sel_g[s0:s0 + chunk], sel_p[s0:s0 + chunk]).sum_d for s0 in range(0, sel_g.shape[0], chunk)]
        return torch.cat(parts) / V

    use_bounds = items >= 1024 if bounds is None else bool(bounds)
    if not use_bounds:
        err_d = (exact(gt_rel, pr_rel) < thr).reshape(hi - lo, n)
        if stats is not None:
            stats.update(items=items, by_bounds=0, exact=items)
        return err_d, err_d.sum(dim=1, dtype=torch.int32)[:, None]
    fld = surface_field(sp)
    lb, ub = ops.adds_bounds(v, gt_rel, pr_rel, fld)
    accept = ub / V < thr - VOTE_SLACK_MM
    reject = lb / V > thr + VOTE_SLACK_MM
    open_idx = torch.nonzero(~(accept | reject))[:, 0]                    # the one host round trip: how many need the search
    err_flat = accept.clone()
    if open_idx.numel():
        err_flat[open_idx] = exact(gt_rel[open_idx], pr_rel[open_idx]) < thr
    if stats is not None:
        stats.update(items=items, by_bounds=items - int(open_idx.numel()), exact=int(open_idx.numel()),
                     accepted_by_bound=int(accept.sum().item()), rejected_by_bound=int(reject.sum().item()))
    err_d = err_flat.reshape(hi - lo, n)
    return err_d, err_d.sum(dim=1, dtype=torch.int32)[:, None]


def vote_choose_image(model_verts, surface_pts, R_gt, t_gt, R_pred, t_pred, diameter, top: int = 50, chunk: int = 4096,
                      bounds: bool | None = None, stats: dict | None = None):
    """choosePose.py:79-151 sharded by rows: every rank holds all n predicted and GT
    poses, builds rows block_range(n, rank, world) of the two relative-pose tables on the device
    (compute_rel_poses, choosePose.py:43-51), evaluates its rows of
        error[i][j] = ADDS(modelVerts, gt_rel[i][j], pred_rel[i][j]) < 0.1 * diameter
    with the batched NN kernel, and all-gathers the int32 row sums; argmax / top-50 are then computed
    identically on every rank (ties -> lower index).  The tables, the ADD-S values and the comparison stay on
    the device: one copy brings back this rank's error rows (the reference writes them to error.npy), one the
    row sums.  bounds / stats: see vote_rows (items decided from the distance field, the search only where needed).  Returns (image_id, top indices, local error rows (rows, n) f64 of 0/1)."""
    rank, size = shard.world()
    n = len(R_gt)
    lo, hi = shard.block_range(n, rank, size)
    dev = registration.device()
    if hi > lo:
        err_d, sums_local = vote_rows(model_verts, surface_pts, R_gt, t_gt, R_pred, t_pred, diameter, lo, hi, chunk, bounds, stats)
        err = err_d.to(torch.float64).cpu().numpy()
    else:
        err = np.zeros((0, n))
        sums_local = torch.zeros((0, 1), dtype=torch.int32, device=dev)
    if size > 1 and shard._coll_device().type == "cpu":
        sums_local = sums_local.cpu()
    sums = shard.allgather_rows(sums_local, n)[:, 0].cpu().numpy().astype(np.float64)
    image_id = int(np.argmax(sums))
    return image_id, np.argsort(-sums, kind="stable")[:top], err


# ------------------------------------------------------------------ icp.py for every listed choice
def pick_refined(fitness, inlier_rmse, n_inliers, chamfer=None):
    """Which refined choice labels the object -> position in the list, or None when none qualifies.
    With final Chamfer values: their FIRST minimum (registration.choose_best's rule, verfication.py:105-106).  Without: the
    highest fitness, then the lowest inlier rmse, then the earliest position.  An item with fewer than 3 correspondences
    (its ICP never moved: no rigid fit exists) or with a NaN in the numbers that decide never wins."""
    fit, rmse = np.asarray(fitness, np.float64), np.asarray(inlier_rmse, np.float64)
    n = np.asarray(n_inliers, np.float64)
    ok = np.isfinite(fit) & np.isfinite(rmse) & (n >= 3)        # a NaN count compares False
    if chamfer is not None:
        c = np.asarray(chamfer, np.float64)
        ok &= np.isfinite(c)
        if not ok.any():
            return None
        return int(np.argmin(np.where(ok, c, np.inf)))
    if not ok.any():
        return None
    best = None
    for i in np.nonzero(ok)[0]:
        if best is None or fit[i] > fit[best] or (fit[i] == fit[best] and rmse[i] < rmse[best]):
            best = int(i)
    return best


def refine_top_choices(upper, lower, R_gt, t_gt, R_pred, t_pred, choices, threshold=20.0, cad_points=None,
                       estimation="point_to_point", target_normals=None, kernel="tukey", k=1.0, **icp_kw):
    """icp.py:37-117 for EVERY image listed in `choices` (the lines of top_50_choices.txt) instead of the first.
    Per choice i: source_i = (upper @ R_gt[i].T + t_gt[i]).astype(float32), formed in f64 on the host (icp.py:68); start
    init_i = inv([R_pred[i] | t_pred[i]]) (icp.py:88-92); target = lower.  One registration.icp_point_to_point_batch for all
    of them, one registration.final_chamfer_batch when cad_points is given; icp_kw goes to the former (max_iter, ...).
    A choice whose predicted pose is a failure (formats.is_failure, or non-finite) is not run: NaN results, iterations -1,
    never best.  Returns a dict: choices (k,) int64, T (k,4,4), fitness, inlier_rmse (k,) f64, iterations (k,) int64,
    chamfer (k,) f64 or None, best (position in choices, pick_refined's rule; None when every choice failed) and
    image_id (choices[best] or None).  choices[0]'s numbers are what icp.py computes today.
    estimation="point_to_plane" runs registration.icp_point_to_plane_batch instead (target_normals: the lower model's,
    None = estimated on the device; kernel and k: the robust weight) and adds "status" (k,) int64, -1 for a choice not
    run; the default, "point_to_point", is unchanged and takes none of the three."""
    from . import formats
    if estimation not in ("point_to_point", "point_to_plane"):
        raise ValueError(f"refine_top_choices: estimation {estimation!r} must be 'point_to_point' or 'point_to_plane'")
    choices = np.asarray(choices, np.int64).reshape(-1)
    weight_k, k = k, len(choices)
    up = np.asarray(upper, np.float64)
    run, srcs, inits = [], [], []
    for pos, i in enumerate(choices):
        R, t = R_pred[i], t_pred[i]
        if formats.is_failure(R, t) or not (np.all(np.isfinite(np.asarray(R, np.float64))) and
                                            np.all(np.isfinite(np.asarray(t, np.float64)))):
            continue
        P = np.vstack([np.hstack([np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)]),
                       [0, 0, 0, 1]])
        run.append(pos)
        srcs.append((up @ np.asarray(R_gt[i], np.float64).T + np.asarray(t_gt[i], np.float64).reshape(3)).astype(np.float32))
        inits.append(np.linalg.inv(P))
    out = {"choices": choices, "T": np.full((k, 4, 4), np.nan), "fitness": np.full(k, np.nan),
           "inlier_rmse": np.full(k, np.nan), "iterations": np.full(k, -1, np.int64),
           "chamfer": None if cad_points is None else np.full(k, np.nan), "best": None, "image_id": None}
    if estimation == "point_to_plane":
        out["status"] = np.full(k, -1, np.int64)
    if not run:
        return out
    srcs = np.stack(srcs)
    if estimation == "point_to_plane":
        T, fit, rmse, iters, out["status"][run] = registration.icp_point_to_plane_batch(
            srcs, lower, threshold, np.stack(inits), target_normals, kernel=kernel, k=weight_k, **icp_kw)
    else:
        T, fit, rmse, iters = registration.icp_point_to_point_batch(srcs, lower, threshold, np.stack(inits), **icp_kw)
    out["T"][run], out["fitness"][run], out["inlier_rmse"][run], out["iterations"][run] = T, fit, rmse, iters
    if cad_points is not None:
        out["chamfer"][run] = registration.final_chamfer_batch(srcs, lower, T, cad_points)
    out["best"] = pick_refined(out["fitness"], out["inlier_rmse"], np.rint(out["fitness"] * up.shape[0]), out["chamfer"])
    out["image_id"] = None if out["best"] is None else int(choices[out["best"]])
    return out


# ------------------------------------------------------------------ the sequence-level pose (include/isr_seq_refit.h)
def stack_correspondences(model: SequenceModel, results: list[ImageResult], pix_xy: torch.Tensor, use: str = "kept"):
    """The 2D-3D matches of every registered frame as one padded block on the device, for joint_transform:
    -> p3d (n, P, 3) f32 model-frame points, p2d (n, P, 2) f32 pixels, counts (n,) i32 (the first counts[i] rows of frame i
    are real).  use="kept": the rows pnp saw (ops.gather_corr's, the top-80 % cut); use="inliers": its consensus set
    (keep[inl_idx[:n_inl]]).  pix_xy (P, 2) shared or (n, P, 2).  A frame whose pnp failed (status 0) gets count 0.  One
    isr_gather_corr_batch launch and tensor plumbing: nothing synchronises, the counts stay on the device."""
    if use not in ("kept", "inliers"):
        raise ValueError(f"stack_correspondences: use {use!r} must be 'kept' or 'inliers'")
    if len(results) == 0:
        raise ValueError("stack_correspondences: no results")
    n = len(results)
    if pix_xy.ndim not in (2, 3) or pix_xy.shape[-1] != 2 or (pix_xy.ndim == 3 and pix_xy.shape[0] != n):
        raise ValueError(f"stack_correspondences: pix_xy {tuple(pix_xy.shape)} must be (P, 2) or ({n}, P, 2)")
    idx = torch.stack([r.idx for r in results])
    keep = torch.stack([r.keep for r in results])
    ok = torch.cat([r.status for r in results]) != 0
    if use == "kept":
        counts = torch.cat([r.M for r in results])
    else:
        P = keep.shape[1]
        inl = torch.stack([r.inl_idx for r in results]).to(torch.int64).clamp_(0, P - 1)     # rows past n_inl are never read
        keep = keep.gather(1, inl).contiguous()
        counts = torch.cat([r.n_inl for r in results])
    counts = torch.where(ok, counts, torch.zeros_like(counts)).to(torch.int32).contiguous()
    p3d, p2d = ops.gather_corr_batch(idx, keep, counts, model.pts, pix_xy)
    return p3d, p2d, counts


def _frames_g(R_gt, t_gt) -> torch.Tensor:
    """(n, 12) f64 [R_i | t_i] on the device."""
    R = registration._dev(np.asarray(R_gt, np.float64) if not isinstance(R_gt, torch.Tensor) else R_gt, torch.float64)
    t = registration._dev(np.asarray(t_gt, np.float64) if not isinstance(t_gt, torch.Tensor) else t_gt, torch.float64)
    n = R.shape[0]
    return torch.cat([R.reshape(n, 3, 3), t.reshape(n, 3, 1)], dim=2).reshape(n, 12).contiguous()


def joint_transform(p3d: torch.Tensor, p2d: torch.Tensor, counts: torch.Tensor, cams, R_gt, t_gt, start, frames=None,
                    kernel: str = "tukey", k: float = 6.0, max_iter: int = 30, tol_r: float = 1e-10, tol_t: float = 1e-8,
                    poses=None) -> dict:
    """The rigid transform Y between the two sequences from EVERY frame's matches (ops.seq_refit): frame i has the known pose
    G_i = [R_gt[i] | t_gt[i]] in its own sequence and sees the first sequence's model under P_i = G_i Y.
    p3d, p2d, counts: stack_correspondences'.  cams: one 3x3 or (n, 3, 3).  start: a 4x4 Y0, or an image id s, which gives
    Y0 = G_s^-1 P_s and needs poses= ((n, 12) or (n, 3, 4) predicted [R|t], e.g. stack_poses(results)[0]).  frames: a boolean
    vector or a list of frame indices that take part (the others weigh 0), e.g. the winner's row of the vote's agreement
    matrix; None: all.  kernel / k: the robust weight on the pixel residual; k = 6 is three times the 2 px inlier bound of
    pnp, so an inlier keeps a weight of at least (1 - 1/9)^2 = 0.79.  Nothing synchronises.  Returns a dict of device tensors:
    Y (4, 4), status, rms, rows, iterations (0-d f64: status 0 converged, 1 max_iter, 2 fewer than 6 rows, 3 singular),
    frame_stats (n, 4) = rows, sum w, sum w r.r, sum r.r per frame at the last pass, and state (24,)."""
    if p3d.ndim != 3:
        raise ValueError(f"joint_transform: p3d {tuple(p3d.shape)} must be (n, cap, 3)")
    n = p3d.shape[0]
    K = np.asarray(cams, np.float64)
    if K.shape not in ((3, 3), (n, 3, 3)):
        raise ValueError(f"joint_transform: cams {K.shape} must be (3, 3) or ({n}, 3, 3)")
    if len(R_gt) != n or len(t_gt) != n:
        raise ValueError(f"joint_transform: {len(R_gt)} R_gt and {len(t_gt)} t_gt for {n} frames")
    frame_w = None
    if frames is not None:
        f = np.asarray(frames)
        if f.dtype == np.bool_:
            if f.shape != (n,):
                raise ValueError(f"joint_transform: a boolean frames must have shape ({n},), got {f.shape}")
            w = f.astype(np.float64)
        else:
            f = f.astype(np.int64).reshape(-1)
            if f.size and (f.min() < 0 or f.max() >= n):
                raise ValueError(f"joint_transform: frames holds an index outside [0, {n})")
            w = np.zeros(n)
            w[f] = 1.0
        frame_w = w
    by_id = isinstance(start, (int, np.integer)) and not isinstance(start, bool)
    if by_id:
        if poses is None:
            raise ValueError("joint_transform: start as an image id needs poses=")
        if not 0 <= int(start) < n:
            raise ValueError(f"joint_transform: start {start} outside [0, {n})")
    else:
        Y0 = start.detach().cpu().numpy() if isinstance(start, torch.Tensor) else np.asarray(start, np.float64)
        if Y0.shape != (4, 4):
            raise ValueError(f"joint_transform: start must be an image id or a 4x4, got shape {Y0.shape}")
    dev = ops.require_cuda(p3d, p2d, counts)
    G = _frames_g(R_gt, t_gt)
    Kd = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(K, (n, 3, 3)).reshape(n, 9))).to(dev)
    state = torch.zeros(24, dtype=torch.float64, device=dev)
    if by_id:
        s = int(start)
        P = registration._dev(poses, torch.float64).reshape(n, 3, 4)[s]
        Rg, tg = G[s].reshape(3, 4)[:, :3], G[s].reshape(3, 4)[:, 3:]
        state[:12] = torch.cat([Rg.T @ P[:, :3], Rg.T @ (P[:, 3:] - tg)], dim=1).reshape(12)      # G_s^-1 P_s, G_s rigid
    else:
        state[:16] = torch.from_numpy(np.ascontiguousarray(Y0, np.float64).reshape(16)).to(dev)
    fw = None if frame_w is None else torch.from_numpy(frame_w).to(dev)
    state, stats = ops.seq_refit(p3d, p2d, counts, Kd, G, state, fw, kernel, k, max_iter, tol_r, tol_t)
    return dict(Y=state[:16].reshape(4, 4), status=state[20], rms=state[17], rows=state[19], iterations=state[18],
                frame_stats=stats, state=state)


def label_frames(Y, R_gt, t_gt) -> tuple[np.ndarray, np.ndarray]:
    """P_i = G_i Y for every frame: the labels of the second sequence in the first sequence's model frame, as
    (R (n, 3, 3), t (n, 3)) f64 host arrays — what formats.write_pred6d_json takes.  Y: a 4x4 (tensor or array)."""
    Y = Y.detach().cpu().numpy() if isinstance(Y, torch.Tensor) else np.asarray(Y)
    Y = np.asarray(Y, np.float64)
    if Y.shape != (4, 4):
        raise ValueError(f"label_frames: Y must be 4x4, got {Y.shape}")
    R = np.asarray(R_gt, np.float64).reshape(-1, 3, 3)
    t = np.asarray(t_gt, np.float64).reshape(-1, 3)
    if len(R) != len(t):
        raise ValueError(f"label_frames: {len(R)} rotations and {len(t)} translations")
    return R @ Y[:3, :3], R @ Y[:3, 3] + t
