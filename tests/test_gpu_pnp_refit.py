"""GPU: the back end of pnp — gn_point / gn_solve on both refit routes (gn_small_kernel up to a capacity of 8192, the
multi-launch gn_accumulate_kernel + gn_solve_kernel above), the inlier mask of the returned pose and its compaction —
against tests/pnp_refit_ref.py: the same iteration in NumPy f64, with the device's retraction, exits and stopping rule, so
that every iteration count has a reference.

Pose tolerance of a case: max(floor, 100 * d_ref), never more than 1e-9 rad / 1e-7 of |t| + 1 (rr.pose_tol).  d_ref is the
distance of the f64 reference from its np.longdouble twin ON THAT CASE; the floor (rr.FLOOR_*) is the largest d_ref that
tests/test_pnp_refit_ref_cpu.py measures — the reference against itself, never the device.  The factor 100 covers what
separates two f64 implementations of one iteration: operation order (fused multiply-adds, the reduction tree), Cholesky
against LU, and a stop one iteration apart when a step lands on the threshold.  (These tests are why gn_solve no longer
damps its diagonal by 1e-14 * trace: with it the device was 1e-6 rad off after one iteration from 15 degrees, 0.16 rad off
after one iteration on an object 6 m away, and 7e-11 rad off there at convergence — see gn_solve.)
Beside the distance every well-posed case asserts cost(device) <= cost(reference) (1 + 1e-9) and, at 10 iterations,
grad_norm(device) <= 100 grad_norm(reference), which do not depend on conditioning.

Within a route results are compared bit for bit: across capacities, padding, unselected rows, batch against single image.
The figures are in profiles/pnp_refit_parity.json (rewritten by running this module with ISR_PNP_REFIT_PARITY_OUT=<file>)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import pnp_refit_ref as rr
from tests import poison

pytestmark = pytest.mark.gpu

REPERR = 2.0
MEASURED = {}


def _record(case, **kw):
    MEASURED.setdefault(case, {}).update({k: [float(x) for x in v] if isinstance(v, tuple) else v for k, v in kw.items()})
    out = os.environ.get("ISR_PNP_REFIT_PARITY_OUT")
    if out:
        what = ("tests/test_gpu_pnp_refit.py: per case d_ref = refine against refine_ext of tests/pnp_refit_ref.py (rad, relative "
                "translation), tol = min(cap, max(floor, factor * d_ref)), device = the device's pose against refine, and the "
                "costs / relative gradient norms behind the other two assertions")
        with open(out, "w") as f:
            json.dump({"what": what, "floor": [rr.FLOOR_ROT, rr.FLOOR_TRANS], "cap": [rr.CAP_ROT, rr.CAP_TRANS], "factor": 100,
                       "cases": MEASURED}, f, indent=1)
            f.write("\n")


def _dev(cuda0, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda0)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _args(s):
    return s["p3d"], s["p2d"], s["K"]


def _padded(s, cap, fill=np.nan):
    """The scene's rows in arrays of `cap` rows; rows at or beyond M hold `fill`."""
    M = len(s["p3d"])
    p3, p2 = np.full((cap, 3), fill, np.float32), np.full((cap, 2), fill, np.float32)
    p3[:M], p2[:M] = s["p3d"], s["p2d"]
    return p3, p2


# ------------------------------------------------------------------------- the multi-launch route: ops.pnp_refine
def _refine_dev(cuda0, p3d, p2d, K, Rt0, words, iters, M=None):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    out = ops.pnp_refine(_dev(cuda0, p3d), _dev(cuda0, p2d), K, _dev(cuda0, Rt0), None if words is None else _dev(cuda0, words),
                         iters=iters, M_dev=M)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_pose(case, got, ref, d, a, sel, iters):
    """The three assertions of a well-posed case; every figure printed and recorded first."""
    tol, dist = rr.pose_tol(d), rr.pose_dist(got, ref)
    cg, cr = rr.cost(*a, got, sel), rr.cost(*a, ref, sel)
    gg, gr = (rr.grad_norm(*a, got, sel), rr.grad_norm(*a, ref, sel)) if iters >= 10 else (None, None)
    print(f"[{case}] d_ref {d[0]:.2e} rad {d[1]:.2e} rel; tol {tol[0]:.1e} {tol[1]:.1e}; device {dist[0]:.2e} {dist[1]:.2e}; "
          f"cost {cg:.15e} / {cr:.15e}; grad {gg} / {gr}")
    _record(case, d_ref=d, tol=tol, device=dist, cost_device=cg, cost_reference=cr, grad_device=gg, grad_reference=gr)
    assert np.all(np.isfinite(got)) and abs(np.linalg.det(got[:, :3]) - 1) < 1e-9
    assert dist[0] <= tol[0] and dist[1] <= tol[1], (case, dist, tol)
    assert cg <= cr * (1 + 1e-9), (case, cg, cr)
    if iters >= 10:
        assert gg <= 100 * gr, (case, gg, gr)


def _check_refit(cuda0, case, s, sel, Rt0, iters):
    got = _refine_dev(cuda0, *_args(s), Rt0, rr.pack_mask(sel), iters)
    _check_pose(case, got, rr.refine(*_args(s), Rt0, sel, iters), rr.d_ref(s, sel, Rt0, iters), _args(s), sel, iters)
    return got


# wave, workgroup and 64-workgroup edges; 16385 / 32769: the second and third trip of the strided loop
SIZES = [4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 16383, 16384, 16385, 32769]


@pytest.mark.parametrize("M", SIZES)
def test_refine_size_edges(cuda0, M):
    s, sel, Rt0 = rr.refine_case("general", 100 + M % 89, M)
    _check_refit(cuda0, f"refine/general/M{M}/it10", s, sel, Rt0, 10)


@pytest.mark.parametrize("iters", [1, 2, 3, 10])
@pytest.mark.parametrize("M", [300, 16385])
def test_refine_partial_counts(cuda0, M, iters):
    """From 15 degrees / 20 mm off, every count against the reference at the same count."""
    s, sel, Rt0 = rr.refine_case("general", 20 + M % 7, M, 15.0, 20.0)
    _check_refit(cuda0, f"refine/general-15deg/M{M}/it{iters}", s, sel, Rt0, iters)


@pytest.mark.parametrize("kind,seed,M", [("planar", 11, 300), ("planar", 9, 4), ("planar", 10, 6), ("far", 12, 300), ("far", 13, 6),
                                         ("few", 1, 4), ("few", 2, 5), ("few", 3, 6)])
def test_refine_geometry(cuda0, kind, seed, M):
    s, sel, Rt0 = rr.refine_case(kind, seed, M)
    _check_refit(cuda0, f"refine/{kind}/M{M}/it10", s, sel, Rt0, 10)


def test_refine_exits_keep_the_pose(cuda0):
    """iters = 0, fewer than 4 selected (0 and 3 bits), and sums that are not finite: the input pose, bit for bit."""
    s, sel, Rt0 = rr.refine_case("general", 5, 300)
    assert _same(_refine_dev(cuda0, *_args(s), Rt0, rr.pack_mask(sel), 0), Rt0)
    three = np.zeros(300, bool)
    three[[3, 170, 299]] = True
    for few_sel in (np.zeros(300, bool), three):
        assert _same(_refine_dev(cuda0, *_args(s), Rt0, rr.pack_mask(few_sel), 10), Rt0)
    four = three.copy()
    four[41] = True                                              # the count is what decides: one more bit and the pose moves
    assert not _same(_refine_dev(cuda0, *_args(s), Rt0, rr.pack_mask(four), 10), Rt0)
    z, zsel, zRt0, m = rr.zc0_case(7, 300)                       # one selected correspondence at z_c = 0 exactly
    assert zsel[m] and rr.gn_step(*_args(z), zRt0, zsel)[0] is None
    got = _refine_dev(cuda0, *_args(z), zRt0, rr.pack_mask(zsel), 10)
    assert np.all(np.isfinite(got)) and _same(got, zRt0)
    zsel[m] = False
    assert not _same(_refine_dev(cuda0, *_args(z), zRt0, rr.pack_mask(zsel), 10), zRt0)


@pytest.mark.parametrize("M,cap", [(257, 300), (8193, 16385), (16385, 20000)])
def test_refine_ignores_padding_and_unselected_rows(cuda0, M, cap):
    s, sel, Rt0 = rr.refine_case("general", 40 + M % 7, M)
    # rows at or beyond M_dev = M hold NaN and every mask word is 0xFFFFFFFF, beyond M too
    words = (cap + 31) // 32
    ones = np.full(words, -1, np.int32)
    alone = _refine_dev(cuda0, *_args(s), Rt0, ones[:(M + 31) // 32], 10)
    p3, p2 = _padded(s, cap)
    assert _same(_refine_dev(cuda0, p3, p2, s["K"], Rt0, ones, 10, M=M), alone)
    assert not _same(alone, Rt0)
    _check_pose(f"refine/padded/M{M}/cap{cap}", alone, rr.refine(*_args(s), Rt0, np.ones(M, bool), 10),
                rr.d_ref(s, np.ones(M, bool), Rt0, 10), _args(s), np.ones(M, bool), 10)
    # NaN in rows inside M that the mask leaves out
    clean = _refine_dev(cuda0, *_args(s), Rt0, rr.pack_mask(sel), 10)
    j3, j2 = s["p3d"].copy(), s["p2d"].copy()
    j3[~sel], j2[~sel] = np.nan, np.nan
    assert _same(_refine_dev(cuda0, j3, j2, s["K"], Rt0, rr.pack_mask(sel), 10), clean) and not _same(clean, Rt0)


def test_refine_does_not_depend_on_capacity(cuda0):
    """refine_impl launches only the workgroups that can own a correspondence: no sum changes with the capacity."""
    M = 5000
    s, sel, Rt0 = rr.refine_case("general", 50, M)
    for iters in (2, 10):
        alone = _refine_dev(cuda0, *_args(s), Rt0, rr.pack_mask(sel), iters)
        assert not _same(alone, Rt0)
        for cap in (8192, 16384, 16385, 40000):
            p3, p2 = _padded(s, cap, 0.0)
            got = _refine_dev(cuda0, p3, p2, s["K"], Rt0, rr.pack_mask(sel, (cap + 31) // 32), iters, M=M)
            assert _same(got, alone), (cap, iters)


def test_refine_collinear_points(cuda0):
    """Singular normal equations (the rotation about the line is free) — properties: a finite proper rotation, and a cost
    that did not rise.  gn_solve KEEPS the pose here (a Cholesky pivot of rounding size, below kGnPivotRel of its
    diagonal entry), which the last assertion pins."""
    for seed, M in ((60, 300), (61, 6)):
        s, sel, Rt0 = rr.refine_case("collinear", seed, M)
        got = _refine_dev(cuda0, *_args(s), Rt0, rr.pack_mask(sel), 10)
        R = got[:, :3]
        c0, c1 = rr.cost(*_args(s), Rt0, sel), rr.cost(*_args(s), got, sel)
        print(f"[refine/collinear/M{M}] cost {c0:.6e} -> {c1:.6e}; moved {rr.pose_dist(got, Rt0)}")
        _record(f"refine/collinear/M{M}/it10", cost_start=c0, cost_device=c1, pose_kept=bool(_same(got, Rt0)))
        assert np.all(np.isfinite(got)) and abs(np.linalg.det(R) - 1) < 1e-9 and np.abs(R @ R.T - np.eye(3)).max() < 1e-9
        assert c1 <= c0, (M, c0, c1)
        assert rr.gn_step(*_args(s), Rt0, sel)[0] is None and _same(got, Rt0), M


# --------------------------------------------------- both routes through pnp_ransac: refit, mask, refit, mask, compaction
def _unpack(r, b=None):
    """Host copy of a PnPResult (poison.to_host) or of image b of a batch."""
    g = (lambda x: x) if b is None else (lambda x: x[b])
    n = int(g(r["n_inl"]).reshape(-1)[0])
    return dict(status=int(g(r["status"]).reshape(-1)[0]), n_eval=int(g(r["n_eval"]).reshape(-1)[0]), n=n,
                idx=g(r["inl_idx"]).numpy()[:n].copy(), pose=g(r["pose"]).numpy().copy())


def _pnp(cuda0, monkeypatch, p3d, p2d, K, H, seed, M=None, **kw):
    """ops.pnp_ransac(loop="sequential") under both poison bytes: what it reports must not depend on what its buffers held."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    d3, d2 = _dev(cuda0, p3d), _dev(cuda0, p2d)
    a, b = poison.run_twice(monkeypatch, lambda: ops.pnp_ransac(d3, d2, K, H=H, reperr=REPERR, seed=seed, M_dev=M,
                                                                loop="sequential", **kw))
    a, b = _unpack(a), _unpack(b)
    assert _same_result(a, b), "the result depends on what the output or scratch buffers held"
    return a


def _same_result(a, b):
    return (a["status"], a["n_eval"], a["n"]) == (b["status"], b["n_eval"], b["n"]) and np.array_equal(a["idx"], b["idx"]) and \
        (a["status"] == 0 or _same(a["pose"], b["pose"]))


def _check_compaction(got, p3d, p2d, K, oracle_lib):
    """inl_idx[:n] is the C oracle's mask of the RETURNED pose, ascending, and n its popcount."""
    if got["status"] == 0:
        assert got["n"] == 0
        return
    m = rr.mask_of(p3d, p2d, K, got["pose"], REPERR, oracle_lib)
    assert got["n"] == int(m.sum()) and np.array_equal(got["idx"], np.nonzero(m)[0])


def _check_pipeline(cuda0, monkeypatch, oracle_lib, case, s, H, seed, iters, cap=None):
    """The device's winner and consensus set (its own refine_iters = 0 run) -> rr.chain -> the device's refitted result."""
    M = len(s["p3d"])
    p3, p2 = _padded(s, cap) if cap else (s["p3d"], s["p2d"])
    Md = M if cap else None
    raw = _pnp(cuda0, monkeypatch, p3, p2, s["K"], H, seed, M=Md, refine_iters=0, inliers="ransac")
    got = _pnp(cuda0, monkeypatch, p3, p2, s["K"], H, seed, M=Md, refine_iters=iters)
    assert raw["status"] == 1 and got["status"] == 1 and raw["n"] >= 4, case
    a = _args(s)
    pose, fin, mid = rr.chain(*a, raw["pose"], raw["idx"], iters, REPERR, oracle_lib)
    _check_pose(case, got["pose"], pose, rr.chain_d_ref(*a, raw["pose"], raw["idx"], mid, iters), a, mid, iters)
    # inliers: the reference's, except correspondences within 1e-3 px of the threshold under the REFERENCE pose
    near = rr.band(*a, pose, REPERR)
    diff = np.setxor1d(got["idx"], np.nonzero(fin)[0])
    _record(case, near_threshold=int(near.sum()), inliers_differ=int(len(diff)), n_inl=got["n"])
    assert near.sum() <= 1, (case, int(near.sum()))               # the seeds were chosen so (on the CPU)
    assert len(diff) <= 2 and np.all(near[diff]), (case, diff)
    _check_compaction(got, *a, oracle_lib)
    return raw, got


# seeds: the first of 300, 301, ... for which the f64 chain from the ORACLE's winner (tests/seq_ransac_ref.py) keeps at least 4
# inliers and has no correspondence within 1e-3 px of the threshold under the first refit and at most one under the second,
# at every iteration count — picked on the CPU, without the device.  6 m away the object is 8 px wide and a 2 px threshold
# passes most outliers, so correspondences near it are common there: hence the later seeds.
_FAR = {33: 300, 257: 303, 5625: 300, 8191: 329, 8192: 324, 8193: 306}
PIPE = [("few", 4, 300), ("few", 5, 300), ("few", 6, 300), ("planar", 4, 300), ("planar", 6, 300), ("far", 4, 300),
        ("far", 6, 300)] + [(k, M, 301 if (k, M) == ("planar", 5625) else _FAR[M] if k == "far" else 300)
                            for k in ("general", "planar", "far") for M in (33, 257, 5625, 8191, 8192, 8193)]
SWITCH_SEED = 300
RAGGED = [("general", 8192, 310), ("general", 257, 311), ("few", 5, 312), ("few", 4, 313)]


@pytest.mark.parametrize("iters", [1, 2, 10])
@pytest.mark.parametrize("kind,M,seed", PIPE)
def test_pipeline_matches_chain(cuda0, monkeypatch, oracle_lib, kind, M, seed, iters):
    """cap = M up to 8192: gn_small_kernel; 8193: the multi-launch route on the same scene family."""
    s = rr.pipeline_scene(kind, seed, M)
    _check_pipeline(cuda0, monkeypatch, oracle_lib, f"pipeline/{kind}/M{M}/it{iters}", s, 500, seed, iters)


def test_route_switch_at_8192(cuda0, monkeypatch, oracle_lib):
    """One 5000-correspondence scene at capacity 8192 (one launch) and 8193 (multi-launch): each against the chain, and
    against each other — poses a rounding apart, inliers equal up to the threshold band."""
    s = rr.pipeline_scene("general", SWITCH_SEED, 5000)
    res = {}
    for cap in (8192, 8193):
        raw, got = _check_pipeline(cuda0, monkeypatch, oracle_lib, f"switch/general/M5000/cap{cap}/it10", s, 500, SWITCH_SEED, 10,
                                   cap=cap)
        res[cap] = (raw, got)
    (ra, ga), (rb, gb) = res[8192], res[8193]
    assert _same_result(ra, rb)                                    # the same winner and consensus set: nothing before the refit differs
    pose, fin, mid = rr.chain(*_args(s), ra["pose"], ra["idx"], 10, REPERR, oracle_lib)
    tol = rr.pose_tol(rr.chain_d_ref(*_args(s), ra["pose"], ra["idx"], mid, 10))
    dist = rr.pose_dist(ga["pose"], gb["pose"])
    _record("switch/general/M5000/it10", tol=tol, across=dist)
    assert dist[0] <= tol[0] and dist[1] <= tol[1], (dist, tol)
    near = rr.band(*_args(s), pose, REPERR)
    diff = np.setxor1d(ga["idx"], gb["idx"])
    assert len(diff) <= 2 and np.all(near[diff]), diff
    # which side of the switch a capacity is on shows in the bits: within a route no sum depends on the capacity, so 8192
    # gives what the scene's own capacity gives (one launch) and 8193 what 16385 gives (multi-launch) ...
    for cap, other in ((8192, None), (8193, 16385)):
        p3, p2 = _padded(s, other) if other else _args(s)[:2]
        o = _pnp(cuda0, monkeypatch, p3, p2, s["K"], 500, SWITCH_SEED, M=5000 if other else None, refine_iters=10)
        assert _same_result(o, res[cap][1]), (cap, other)
    # ... and the two routes sum in different orders: were one capacity on the wrong side, these would be the same bits
    assert not _same(ga["pose"], gb["pose"])


@pytest.mark.parametrize("cap", [8192, 16385])
def test_ragged_batch_equals_single_images(cuda0, oracle_lib, cap):
    """M_dev = [8192, 257, 5, 4, 3] in one batch: every image's outputs are those of the image alone at the same capacity,
    bit for bit — and, on the one-launch route, of the image alone at ITS OWN capacity (gn_small_kernel's sums do not depend
    on the capacity).  The last image has no pose.  Rows beyond M_dev hold NaN."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    scenes = [rr.pipeline_scene(k, seed, M) for k, M, seed in RAGGED]
    rng = np.random.default_rng(5)
    scenes.append(dict(K=scenes[0]["K"], p3d=rng.normal(0, 30, (3, 3)).astype(np.float32),
                       p2d=rng.uniform(0, 100, (3, 2)).astype(np.float32)))
    B = len(scenes)
    Ms = np.array([len(s["p3d"]) for s in scenes], np.int32)
    pads = [_padded(s, cap) for s in scenes]
    d3, d2 = _dev(cuda0, np.stack([p[0] for p in pads])), _dev(cuda0, np.stack([p[1] for p in pads]))
    M_dev = _dev(cuda0, Ms)
    seeds = [s_[2] for s_ in RAGGED] + [0]
    kw = dict(H=500, reperr=REPERR, loop="sequential")
    for iters in (2, 10):
        r = ops.pnp_ransac_batch(d3, d2, scenes[0]["K"], M_dev, seeds=seeds, refine_iters=iters, **kw)
        torch.cuda.synchronize()
        r = poison.to_host(r)
        for b in range(B):
            got = _unpack(r, b)
            one = ops.pnp_ransac(d3[b], d2[b], scenes[b]["K"], seed=seeds[b], M_dev=M_dev[b:b + 1], refine_iters=iters, **kw)
            torch.cuda.synchronize()
            assert _same_result(got, _unpack(poison.to_host(one))), (cap, iters, b)
            assert got["status"] == (0 if Ms[b] < 4 else 1), (cap, iters, b)
            if got["status"]:
                _check_compaction(got, *_args(scenes[b]), oracle_lib)
            if cap <= 8192:
                own = ops.pnp_ransac(_dev(cuda0, scenes[b]["p3d"]), _dev(cuda0, scenes[b]["p2d"]), scenes[b]["K"], seed=seeds[b],
                                     refine_iters=iters, **kw)
                torch.cuda.synchronize()
                assert _same_result(got, _unpack(poison.to_host(own))), (cap, iters, b, "own capacity")


# ------------------------------------------------------------------------------------------------ compaction
# 256 mask words (8192 correspondences) per compaction block: one block full, one bit short, one bit over, three blocks
@pytest.mark.parametrize("M", [8191, 8192, 8193, 16385])
@pytest.mark.parametrize("fill", ["all", "few", "none"])
def test_compaction_block_edges(cuda0, monkeypatch, oracle_lib, M, fill):
    if fill == "all":        # exact pixels, no outliers: every correspondence is an inlier of the returned pose
        s = rr.pipeline_scene("general", 320, M, clean=True)
        got = _pnp(cuda0, monkeypatch, *_args(s), 500, 320, refine_iters=10)
        assert got["status"] == 1 and np.array_equal(got["idx"], np.arange(M))
    elif fill == "few":      # 85 % outliers
        s = rr.pipeline_scene("general", 321, M, outlier_frac=0.85)
        got = _pnp(cuda0, monkeypatch, *_args(s), 2000, 321, refine_iters=10)
        assert got["status"] == 1 and 0.1 * M < got["n"] < 0.2 * M
        assert rr.pose_dist(got["pose"], s["Rt"])[0] < 3e-3
    else:                    # no pose at all
        s = rr.pipeline_scene("noise", 322, M)
        got = _pnp(cuda0, monkeypatch, *_args(s), 500, 322, refine_iters=10)
        assert got["status"] == 0 and got["n"] == 0
    _check_compaction(got, *_args(s), oracle_lib)


def test_compaction_at_245760(cuda0, monkeypatch, oracle_lib):
    """30 compaction blocks, the scan of their totals: inl_idx is the mask of the returned pose here too."""
    M = 245760
    s = rr.pipeline_scene("general", 323, M)
    got = _pnp(cuda0, monkeypatch, *_args(s), 500, 323, refine_iters=10)
    assert got["status"] == 1 and got["n"] > 0.95 * s["inl"].sum() and rr.pose_dist(got["pose"], s["Rt"])[0] < 3e-3
    _check_compaction(got, *_args(s), oracle_lib)
