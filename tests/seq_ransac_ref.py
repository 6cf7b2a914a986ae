"""Test helper (not collected): OpenCV's sequential RANSAC loop, literally, for ops.pnp_ransac(loop="sequential").

cv2.solvePnPRansac runs RANSACPointSetRegistrator::run with RANSACUpdateNumIters (calib3d; restated from memory, OpenCV
is not installed):

    niters = itr; best = 0
    for h = 0, 1, ...  while h < niters:
        if hypothesis h has a model and count[h] > max(best, 3):
            best = count[h]; winner = h
            niters = update(confidence, ep = (M - best) / M, 4, niters)

`update_log` is cv2's update (log / pow, cvRound = round half to even); `update_exact` decides the same rounding with
multiplications and one sqrt, operation for operation csrc/ransac_seq.hpp:seq_stop.  `closed_form` is the parallel form
the device kernel uses (h_stop = the first h at which the loop stops given the prefix maximum before it).
`pnp_ransac_seq` is the whole call: oracle hypotheses, every one scored by the C oracle, the loop replayed on the counts,
the winner's consensus set, and the same two refit rounds as oracle/pnp_oracle.py:pnp_ransac.
"""
from __future__ import annotations

import math
import sys

import numpy as np

DBL_MIN = sys.float_info.min


def seq_num(confidence: float) -> float:
    n = 1.0 - float(confidence)
    return n if n > DBL_MIN else DBL_MIN


def _d(c: int, M: int) -> float:
    ep = float(M - c) / float(M)
    t = 1.0 - ep
    t2 = t * t
    return 1.0 - t2 * t2


def seq_stop(c: int, M: int, h: int, num: float) -> bool:
    """csrc/ransac_seq.hpp:seq_stop, operation for operation (IEEE doubles)."""
    if c <= 3 or M <= 0:
        return False
    d = _d(c, M)
    if d < DBL_MIN:
        return True
    if not d < 1.0:
        return False
    base, q, e = d, 1.0, int(h)
    while e > 0:
        if e & 1:
            q = q * base
        base = base * base
        e >>= 1
    return num >= q * math.sqrt(d)


def update_exact(confidence: float, M: int, c: int, n: int) -> int:
    """niters after a new best count c: the first h < n at which seq_stop holds, else n."""
    num = seq_num(confidence)
    d = _d(c, M)
    if d < DBL_MIN:
        return 0
    if not d < 1.0:
        return n
    h = min(n, max(0, int(math.log(num) / math.log(d))))     # a start near the answer; the predicate decides
    while h > 0 and seq_stop(c, M, h - 1, num):
        h -= 1
    while h < n and not seq_stop(c, M, h, num):
        h += 1
    return h


def update_log(confidence: float, M: int, c: int, n: int) -> int:
    """RANSACUpdateNumIters(confidence, (M - c) / M, 4, n) as cv2 writes it."""
    ep = float(M - c) / float(M)
    num = max(1.0 - float(confidence), DBL_MIN)
    den = 1.0 - math.pow(1.0 - ep, 4)
    if den < DBL_MIN:
        return 0
    num, den = math.log(num), math.log(den)
    if den >= 0 or -num >= n * (-den):
        return n
    return int(round(num / den))


def log_ratio(confidence: float, M: int, c: int) -> float:
    """log(num) / log(den) of cv2's update (inf when den rounds to 1)."""
    den = 1.0 - math.pow(float(c) / float(M), 4)
    if den < DBL_MIN:
        return 0.0
    if den >= 1.0:
        return math.inf
    return math.log(max(1.0 - float(confidence), DBL_MIN)) / math.log(den)


def literal_loop(counts, ok, M: int, itr: int, confidence: float, update=update_exact) -> tuple[int, int]:
    """-> (winner, n_eval): the loop above, niters recomputed at every new best."""
    niters, best, winner, h = int(itr), 0, -1, 0
    while h < niters:
        if ok[h] and int(counts[h]) > max(best, 3):
            best, winner = int(counts[h]), h
            niters = update(confidence, M, best, niters)
        h += 1
    return winner, h


def seq_stop_vec(c, M: int, h, num: float):
    """seq_stop over arrays of (c, h), the same operations element by element."""
    c = np.asarray(c, np.int64)
    h = np.asarray(h, np.int64)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        ep = (np.float64(M) - c.astype(np.float64)) / np.float64(M) if M > 0 else np.zeros(c.shape)
        t = 1.0 - ep
        t2 = t * t
        d = 1.0 - t2 * t2
        base, q, e = d.copy(), np.ones(d.shape), h.copy()
        while np.any(e > 0):
            q = np.where(e & 1, q * base, q)
            base = base * base
            e >>= 1
        out = num >= q * np.sqrt(np.maximum(d, 0.0))
    out = np.where(d < DBL_MIN, True, out)
    out = np.where(d < 1.0, out, False)
    return np.where((c <= 3) | (M <= 0), False, out)


def closed_form(counts, ok, M: int, itr: int, confidence: float) -> tuple[int, int]:
    """The parallel form: h_stop = the first h with seq_stop(max count before h, M, h), else itr; winner = the lowest h
    with the maximal count (> 3) in [0, h_stop)."""
    v = np.where(np.asarray(ok[:itr]).astype(bool), np.asarray(counts[:itr], np.int64), 0)
    H = len(v)
    if H == 0:
        return -1, 0
    before = np.concatenate([[0], np.maximum.accumulate(v)[:-1]])
    stop = seq_stop_vec(before, M, np.arange(H), seq_num(confidence))
    h_stop = int(np.argmax(stop)) if stop.any() else H
    if h_stop == 0 or v[:h_stop].max() <= 3:
        return -1, h_stop
    return int(np.argmax(v[:h_stop])), h_stop


def pnp_ransac_seq(p3d, p2d, K, H=500, reperr=2.0, seed=0, refine_iters=10, confidence=0.99, hyp=None):
    """The sequential loop over the oracle's hypotheses (or `hyp` = (Rt (H,3,4), ok (H,)) given) ->
    dict(status, winner, n_eval, consensus (RANSAC inliers, ascending), inliers (of the refitted pose), Rt, n_inl)."""
    from oracle import cbind
    from oracle import pnp_oracle as po
    p3d = np.ascontiguousarray(p3d, np.float32)
    p2d = np.ascontiguousarray(p2d, np.float32)
    K = np.asarray(K, np.float64)
    M = len(p3d)
    Rt, ok = hyp if hyp is not None else po.hypotheses(p3d, p2d, K, H, seed)[:2]
    Rt = np.asarray(Rt, np.float64).reshape(H, 3, 4)
    ok = np.asarray(ok, np.uint8)
    sc = cbind.ransac_score(p3d, p2d, K, Rt, ok, reperr)               # every hypothesis scored, then replayed
    winner, n_eval = literal_loop(sc["n_inl"], ok, M, H, confidence)
    status = int(winner >= 0)
    empty = np.zeros(0, np.int32)
    if not status:
        return dict(status=0, winner=-1, n_eval=n_eval, consensus=empty, inliers=empty, Rt=np.eye(3, 4), n_inl=sc["n_inl"])

    def mask_of(T):
        m = cbind.ransac_score(p3d, p2d, K, np.asarray(T).reshape(1, 12), np.ones(1, np.uint8), reperr)["best_mask"]
        return po.unpack_mask(m, M)

    cons = mask_of(Rt[winner])
    pose, inl = Rt[winner], cons
    if refine_iters > 0:
        pose = po.refine(p3d, p2d, K, pose, inl, refine_iters)
        pose = po.refine(p3d, p2d, K, pose, mask_of(pose), refine_iters)
        inl = mask_of(pose)
    return dict(status=1, winner=winner, n_eval=n_eval, consensus=np.nonzero(cons)[0].astype(np.int32),
                inliers=np.nonzero(inl)[0].astype(np.int32), Rt=pose, n_inl=sc["n_inl"])
