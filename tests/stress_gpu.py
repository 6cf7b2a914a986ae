"""Randomised stress of the HIP path against the C oracle (a script, not collected by pytest: minutes, not seconds).
    python tests/stress_gpu.py [seed] [cases]
Round 5: tools/stress_corr_screened.py found a tie-order bug no fixed-size test held; this is the same net under the other
routes of K1 and under the nearest-neighbour search.  Per case random shapes (ragged), random composition of rows:
  corr   f32 / bf16 / bf16-log2 routes of isr_corr_argmax, D in 1..128, planted / unplanted / zero / huge / tiny / duplicated rows:
         indices array_equal to the oracle's exact arg-max (lowest key on ties); logp and lse to 3e-5 (relative to
         max(1, |lse|)); a random slice of the queries in a launch of its own: indices torch.equal, values torch.equal for
         the queries inside the direct sums' range.
  nn     isr_nn_batched with random transforms, radius, lattice clouds (exact ties), duplicated targets: winners and f64
         distances bit for bit, counts equal, sums to 1e-12.
  ransac random M (4 ...), H, thresholds, outlier fractions, pixel-rounded observations: Philox samples array_equal to the numpy
         oracle's; inlier counts, best hypothesis and its bit mask array_equal to the C oracle's on the device's own poses.
  filter the top-80 % cut on exponential / plateau / half-zero / -inf log-probabilities, 2 ... 400 000 values: kept set array_equal
         to inference.py:282-290 restated.
  icp    random cloud sizes (3 ...), initial poses, thresholds (few / all points inside), Morton order on and off: fitness equal,
         rmse to 1e-9, pose to 1e-9 rad / 1e-7 mm of the oracle loop with exact f64 neighbours.
  crop   the image front end (inference.py:196-232): random frame sizes and masks (boxes touching the frame, one pixel, scattered
         pixels, the whole frame, grey-valued ellipses), with and without blanking: bounding box, affine map, warped mask bytes and
         normalised network input array_equal to the numpy oracle.
  prep   the network-output -> K1 hand-off (inference.py:248-279): random sizes from 1 x 1, strides, mask channel layouts and
         densities (empty, full), three row formats: row count, pixel coordinates and rows bit for bit, padding rows zero.
  pose   relative-pose tables (choosePose.py:43-51, verfication.py:9-19) to 1e-9 relative, ADD to 1e-9, ADD-S to 1e-6 (f32 winners,
         f64 distances against sklearn's KD-tree) on random poses and clouds.
  vote / pick  the n x n ADD-S vote with and without the distance-field bounds (every decision farther than 1e-6 mm from the threshold
         equal to choosePose.py:121-145's) and the consecutive-pair Chamfer pick (verfication.py:61-108) to 1e-9.
  pnp    the fused PnP + RANSAC call on random sizes (4 ...), hypothesis counts, confidences, thresholds and outlier fractions
         (to 85 %): hypotheses scored, inlier set and pose (1e-4 rad / 1e-3 mm) against oracle/pnp_oracle.py.
  batch cut  the cut + assembly of a group of images with ragged device-side counts (0, 1, 2, 500, 501, P among them) against
         inference.py:274-290 per image; K1's lse-only call against the full call's lse, torch.equal.
  bounds the distance-field brackets of the vote (isr_adds_bounds) contain the exact ADD-S sums: random clouds, grids of 16-128 cells,
         poses orthonormal to f32 only, vertices hundreds of millimetres off the grid."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops  # noqa: E402
from oracle import cbind  # noqa: E402

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
cases = int(sys.argv[2]) if len(sys.argv) > 2 else 60
dev = torch.device("cuda:0")
rng = np.random.default_rng(seed)
cbind.build()


def bits(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def corr_case(c):
    route = str(rng.choice(["f32", "bf16", "log2"]))
    D = int(rng.choice([rng.integers(1, 129), 64, 64, 32, 128, 16]))
    P = int(rng.integers(1, 6000))
    N = int(rng.choice([rng.integers(1, 300), rng.integers(300, 5000), rng.integers(5000, 30000)]))
    tau = float(rng.choice([0.5, 2.0, 5.0, 8.0, 12.0]))
    K = rng.normal(0, 1, (N, D)).astype(np.float32)
    K *= tau / np.maximum(np.linalg.norm(K, axis=1, keepdims=True), 1e-6)
    if N > 10 and rng.random() < 0.5:
        j = rng.integers(N, size=N // 10); i = rng.integers(N, size=N // 10)
        K[j] = K[i] * (1.0 + rng.choice([0.0, 1e-3, 1e-2], size=(N // 10, 1)))
    gt = rng.integers(N, size=P)
    Q = (K[gt] + float(rng.choice([0.05, 0.35, 1.0])) * rng.normal(0, 1, (P, D))).astype(np.float32)
    kind = rng.random(P)
    Q[kind < 0.15] = rng.normal(0, 1, (int((kind < 0.15).sum()), D))
    Q[(kind > 0.15) & (kind < 0.20)] = 0.0
    Q[(kind > 0.20) & (kind < 0.23)] *= 10.0
    Q[(kind > 0.23) & (kind < 0.26)] *= 1e-3
    tag = f"corr case {c}: {route} P={P} N={N} D={D} tau={tau}"
    if route == "f32":
        q, k = torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev)
        g = ops.corr_argmax(q, k, want_lse=True)
        o = cbind.corr_argmax_f32(Q, K)
        mx, lse_o = o["maxlogit"].astype(np.float64), o["lse"]
        kw = {}
    else:
        qb = ops.prescale_queries_log2(torch.from_numpy(Q)) if route == "log2" else torch.from_numpy(Q).bfloat16()
        kb = torch.from_numpy(K).bfloat16()
        q, k = qb.to(dev), kb.to(dev)
        kw = dict(log2_prescaled=route == "log2")
        g = ops.corr_argmax(q, k, want_lse=True, **kw)
        o = cbind.corr_argmax_bf16(bits(qb), bits(kb), logit_scale=np.log(2.0) if route == "log2" else 1.0)
        mx, lse_o = o["maxlogit"], o["lse"]
    idx, logp, lse = (x.cpu().numpy() for x in g)
    bad = np.nonzero(idx != o["idx"])[0]
    assert len(bad) == 0, f"{tag}: {len(bad)} index mismatches, first {bad[:4]}, margins {(mx - o['top2'])[bad][:4]}"
    scale = np.maximum(1.0, np.abs(lse_o))
    e1 = np.max(np.abs(lse - lse_o) / scale)
    e2 = np.max(np.abs(logp - (mx - lse_o)) / scale)
    assert e1 <= 3e-5 and e2 <= 3e-5, f"{tag}: lse off by {e1:.3g}, logp by {e2:.3g}"
    lo = int(rng.integers(0, P)); hi = min(P, lo + int(rng.integers(1, 2000)))
    s = ops.corr_argmax(q[lo:hi].contiguous(), k, want_lse=True, **kw)
    # (a query whose logits leave the direct sums' range, |log2-unit logit| >= 100 here, is still decided exactly, but which of
    # its key ranges are redone with a per-query reference — and with that the last bit of its values — follows the launch's
    # key split: DESIGN.md K1a "launch independence")
    inr = torch.from_numpy((np.abs(mx[lo:hi]) * 1.4427 < 100.0) & (np.abs(lse_o[lo:hi]) * 1.4427 < 100.0)).to(dev)
    assert torch.equal(g[0][lo:hi], s[0]), f"{tag}: slice [{lo}, {hi}) indices differ"
    assert all(torch.equal(x[lo:hi][inr], y[inr]) for x, y in zip(g, s)), f"{tag}: slice [{lo}, {hi}) differs"
    return max(e1, e2)


def rand_pose():
    a = rng.normal(0, 1, 4); a /= np.linalg.norm(a)
    w, x, y, z = a
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.concatenate([R, rng.normal(0, 30, (3, 1))], axis=1)


def nn_case(c):
    Nq = int(rng.choice([rng.integers(1, 200), rng.integers(200, 6000)]))
    Nt = int(rng.choice([rng.integers(1, 300), rng.integers(300, 9000)]))
    B = int(rng.choice([1, 1, 2, 5, 17]))
    lattice = rng.random() < 0.3
    if lattice:
        q = rng.integers(-4, 5, (Nq, 3)).astype(np.float32)
        t = rng.integers(-4, 5, (Nt, 3)).astype(np.float32)
    else:
        q = rng.normal(0, 40, (Nq, 3)).astype(np.float32)
        t = rng.normal(0, 40, (Nt, 3)).astype(np.float32)
        if Nt > 4 and rng.random() < 0.5:
            t[Nt // 2:] = t[: Nt - Nt // 2]
    mode = int(rng.integers(0, 4))
    Tq = np.stack([rand_pose() for _ in range(B)]) if (mode & 1 or B > 1) else None
    Tt = np.stack([rand_pose() for _ in range(B)]) if (mode & 2 and not lattice) else None
    if lattice and Tq is not None:                           # keep the ties exact: integer translations, axis permutations
        Tq = np.stack([np.concatenate([np.eye(3)[rng.permutation(3)], rng.integers(-2, 3, (3, 1)).astype(float)], axis=1)
                       for _ in range(B)])
    if Tq is None and Tt is not None and B > 1:
        Tq = np.stack([np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)] * B)
    radius = float(rng.choice([-1.0, 3.0, 20.0, 60.0]))
    tag = f"nn case {c}: Nq={Nq} Nt={Nt} B={B} lattice={lattice} radius={radius} Tq={Tq is not None} Tt={Tt is not None}"
    r = ops.nn_batched(torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev),
                       None if Tq is None else torch.from_numpy(Tq).to(dev), None if Tt is None else torch.from_numpy(Tt).to(dev),
                       radius=radius, want_idx=True, want_dist=True, want_cov=True)
    g = {k: getattr(r, k).cpu().numpy() for k in ("sum_d", "sum_d2", "n_in", "nn_idx", "nn_d")}
    o = cbind.nn_batched(q, t, Tq, Tt, radius)
    assert np.array_equal(g["nn_idx"], o["nn_idx"]), f"{tag}: {(g['nn_idx'] != o['nn_idx']).sum()} winners differ"
    assert np.array_equal(g["nn_d"], o["nn_d"]), f"{tag}: distances differ"
    assert np.array_equal(g["n_in"], o["n_in"]), f"{tag}: counts differ"
    np.testing.assert_allclose(g["sum_d"], o["sum_d"], rtol=1e-12, err_msg=tag)
    np.testing.assert_allclose(g["sum_d2"], o["sum_d2"], rtol=1e-12, err_msg=tag)


def ransac_case(c):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import synth
    from oracle import pnp_oracle as po
    M = int(rng.choice([rng.integers(4, 100), rng.integers(100, 5000), rng.integers(5000, 60000)]))
    H = int(rng.choice([1, 7, 64, 500, 1000]))
    sd = int(rng.integers(1 << 31))
    reperr = float(rng.choice([0.5, 2.0, 8.0]))
    pts = synth.tless_like(rng, 2000)
    Kc = synth.camera()
    R, t = synth.random_poses(rng, 1)
    p3d, p2d, _ = synth.pnp_case(rng, pts, Kc, R[0], t[0], M, float(rng.choice([0.0, 0.5, 2.0])), float(rng.choice([0.0, 0.3, 0.9])))
    if rng.random() < 0.3:
        p2d = np.round(p2d)                                   # pixel centres: reprojection errors that tie across hypotheses
    tag = f"ransac case {c}: M={M} H={H} reperr={reperr}"
    d3, d2 = torch.from_numpy(p3d).to(dev), torch.from_numpy(p2d).to(dev)
    Rt, ok, smp = ops.p3p_hypotheses(d3, d2, Kc, H, seed=sd, want_samples=True)
    n_inl, best, mask = ops.ransac_score(d3, d2, Kc, Rt, ok, reperr)
    assert np.array_equal(smp.cpu().numpy(), po.sample_indices(H, M, sd)), f"{tag}: samples differ"
    Rt_h, ok_h = Rt.cpu().numpy(), ok.cpu().numpy()
    sc = cbind.ransac_score(p3d, p2d, Kc, Rt_h.reshape(H, 12), ok_h, reperr)
    assert np.array_equal(n_inl.cpu().numpy(), sc["n_inl"]), f"{tag}: inlier counts differ"
    assert int(best.item()) == sc["best"], f"{tag}: best differs"
    assert np.array_equal(mask.cpu().numpy().view(np.uint32), sc["best_mask"]), f"{tag}: mask differs"


def filter_case(c):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import registration as reg
    from oracle import registration_oracle as ro
    P = int(rng.choice([rng.integers(2, 501), rng.integers(501, 3000), rng.integers(3000, 400000)]))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        x = -rng.exponential(3.0, P)
    elif kind == 1:
        x = -rng.integers(0, 6, P).astype(np.float64)          # plateaus: the threshold sits inside a run of equal values
    elif kind == 2:
        x = -np.abs(rng.normal(0, 1e-6, P)); x[rng.random(P) < 0.5] = 0.0     # the bench's tau = 8 case: half the values are 0
    else:
        x = -rng.exponential(3.0, P); x[rng.random(P) < 0.01] = -np.inf
    x = x.astype(np.float32)
    tag = f"filter case {c}: P={P} kind={kind}"
    got = reg.filter_top(torch.from_numpy(x).to(dev).reshape(-1, 1))
    want = ro.filter_top(torch.from_numpy(x).reshape(-1, 1))
    assert np.array_equal(got, want), f"{tag}: kept sets differ ({len(got)} vs {len(want)})"


def icp_case(c):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import registration as reg, synth
    from oracle import registration_oracle as ro
    n = int(rng.choice([rng.integers(3, 300), rng.integers(300, 3000), rng.integers(3000, 9000)]))
    m = int(rng.choice([n, rng.integers(3, 9000)]))
    cloud = synth.bumpy_ellipsoid(rng, 4 * max(n, m)) if rng.random() < 0.5 else synth.tless_like(rng, 4 * max(n, m))
    src = cloud[rng.choice(len(cloud), n, replace=False)].astype(np.float32)
    tgt = cloud[rng.choice(len(cloud), m, replace=False)].astype(np.float32)
    ang = float(rng.choice([0.0, 0.01, 0.05, 0.3]))
    ax = rng.normal(0, 1, 3); ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    init = np.eye(4)
    init[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    init[:3, 3] = rng.normal(0, float(rng.choice([0.0, 0.5, 3.0])), 3)
    thr = float(rng.choice([0.5, 5.0, 20.0, 200.0]))
    tag = f"icp case {c}: n={n} m={m} angle={ang} threshold={thr}"
    T, fit, rmse = reg.icp_point_to_point(src, tgt, thr, init, spatial_order=bool(rng.random() < 0.5))
    Tr, rfit, rrmse, traj = ro.icp_point_to_point(src, tgt, thr, init, search="f64")
    # the loop is a fixed point iteration: a neighbour decided differently at a tie of f32 roundings would show as a different
    # trajectory; the device resolves such ties in f64, so the poses agree to the conditioning of the last Kabsch step
    rot = synth.rot_angle(T[:3, :3], Tr[:3, :3]); tr = float(np.linalg.norm(T[:3, 3] - Tr[:3, 3]))
    assert abs(fit - rfit) < 1e-12 and abs(rmse - rrmse) < 1e-9 * max(1.0, rrmse) and rot < 1e-9 and tr < 1e-7, \
        f"{tag}: fitness {fit} / {rfit}, rmse {rmse} / {rrmse}, rot {rot:.3g} rad, trans {tr:.3g} mm after {len(traj) - 1} iterations"
    return rot


def crop_case(c):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import formats, registration as reg
    from oracle import preprocess_oracle as pp
    H, W = int(rng.integers(40, 500)), int(rng.integers(40, 660))
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    mask = np.zeros((H, W, 3), np.uint8)
    kind = int(rng.integers(0, 5))
    if kind == 0:                                                # a box anywhere, frame-touching ones included
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        mask[y0:y0 + int(rng.integers(1, H)), x0:x0 + int(rng.integers(1, W))] = 255
    elif kind == 1:                                              # one pixel (a corner one time in two)
        y, x = (int(rng.choice([0, H - 1])), int(rng.choice([0, W - 1]))) if rng.random() < 0.5 else (int(rng.integers(H)), int(rng.integers(W)))
        mask[y, x] = int(rng.integers(1, 256))
    elif kind == 2:                                              # scattered pixels
        mask[rng.random((H, W)) < 0.002] = 255
    elif kind == 3:                                              # the whole frame
        mask[:] = 255
    else:                                                        # an ellipse with grey edge values
        yy, xx = np.mgrid[0:H, 0:W]
        inside = ((xx - W * rng.random()) / (W * 0.3 + 1)) ** 2 + ((yy - H * rng.random()) / (H * 0.3 + 1)) ** 2 <= 1.0
        mask[inside] = rng.integers(1, 256, size=(int(inside.sum()), 1))
    use_mask = bool(rng.random() < 0.7)
    tag = f"crop case {c}: {H}x{W} kind={kind} use_mask={use_mask}"
    bb = pp.bounding_rect(mask[:, :, 0])
    got_bb = tuple(ops.mask_bbox(torch.from_numpy(mask[None]).to(dev)).cpu().numpy()[0])
    assert got_bb == bb, f"{tag}: bbox {got_bb} / {bb}"
    if bb[2] == 0 or bb[3] == 0:
        return
    Kc = np.array([[1075.65, 0, W / 2], [0, 1073.9, H / 2], [0, 0, 1]])
    if max(bb[2] - bb[2] % 2, bb[3] - bb[3] % 2) == 0:           # a 1 x 1 box: inference.py:203-215 divides by max(w, h) = 0
        try:
            reg.crop_inputs(rgb, mask, Kc, useMask=use_mask)
        except ZeroDivisionError:
            return
        raise AssertionError(f"{tag}: the reference raises ZeroDivisionError for a 1 x 1 box")
    inputIM, cropMask, cam, M = reg.crop_inputs(rgb, mask, Kc, useMask=use_mask)
    assert np.array_equal(M[0], formats.crop_affine(bb)), f"{tag}: M differs"
    ref_in, ref_mask = pp.crop_inputs(rgb, mask, M[0], 224, use_mask)
    assert np.array_equal(cropMask[0].cpu().numpy(), ref_mask), f"{tag}: crop mask differs"
    assert np.array_equal(inputIM[0].cpu().numpy(), ref_in), f"{tag}: network input differs"


def prep_case(c):
    """inference.py:248-279 literally (torch CPU) against ops.prep_queries."""
    H, W = int(rng.integers(1, 260)), int(rng.integers(1, 260))
    C = int(rng.integers(12, 24)); ds = int(rng.choice([1, 2, 3, 4])); ch = int(rng.choice([0, 1, 3]))
    dtype = str(rng.choice(["f32", "bf16", "bf16_log2"]))
    feat = torch.from_numpy(rng.normal(0, 2, (1, H, W, C)).astype(np.float32))
    m = (rng.random((H, W)) < float(rng.choice([0.0, 0.02, 0.5, 1.0]))).astype(np.uint8) * int(rng.integers(1, 256))
    mask = torch.from_numpy(np.repeat(m[:, :, None], ch, axis=2) if ch else m)
    tag = f"prep case {c}: {H}x{W}x{C} step {ds} mask channels {ch} {dtype}"
    imfeats = feat[..., 0:12][:, ::ds, ::ds]
    inputMask = (mask[:, :, 0] if mask.ndim == 3 else mask)[::ds, ::ds]
    ids = torch.where(inputMask)
    mf = imfeats[0][ids]
    Q, pix, n_dev = ops.prep_queries(feat.to(dev), mask.to(dev), c0=0, D=12, step=ds, dtype=dtype)
    n = int(n_dev.item())
    assert n == mf.shape[0], f"{tag}: {n} rows / {mf.shape[0]}"
    got = pix[:n].cpu().numpy()
    assert np.array_equal(got[:, 0], ids[1].numpy()) and np.array_equal(got[:, 1], ids[0].numpy()), f"{tag}: pixel coordinates differ"
    Qh = Q.cpu()
    if dtype == "f32":
        assert torch.equal(Qh[:n], mf), f"{tag}: rows differ"
    else:
        want = ops.prescale_queries_log2(mf) if dtype == "bf16_log2" else mf.bfloat16()
        assert torch.equal(Qh[:n, :12].view(torch.int16), want.view(torch.int16)), f"{tag}: rows differ"
    assert (Qh[n:].float() == 0).all(), f"{tag}: padding rows are not zero"


def pose_case(c):
    """choosePose.py:43-51 / 98-107, verfication.py:9-19, inference.py:116-120 against the device tables and metrics."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import registration as reg
    from oracle import registration_oracle as ro
    n = int(rng.integers(1, 12))
    T = [rand_pose() for _ in range(n)]
    R = np.stack([t[:, :3] for t in T]); t = np.stack([t[:, 3] + np.array([0, 0, 600.0]) for t in T])
    for mode, fn in (("choose", ro.compute_rel_poses), ("verif", ro.calculate_relative_pose)):
        got = reg.relative_pose_table(R, t, mode=mode)
        want = ro.rel_pose_table(R, t, fn)
        assert np.allclose(got, want, rtol=0, atol=1e-9 * 600.0), f"pose case {c}: table '{mode}' differs by {np.abs(got - want).max():.3g}"
    nv, ns = int(rng.integers(1, 3000)), int(rng.integers(1, 4000))
    verts = rng.normal(0, 30, (nv, 3)).astype(np.float32)
    surf = rng.normal(0, 30, (ns, 3)).astype(np.float32)
    i, j = int(rng.integers(n)), int(rng.integers(n))
    a = reg.ADD(verts, R[i], t[i], R[j], t[j]); ar = ro.ADD(verts.astype(np.float64), R[i], t[i], R[j], t[j])
    assert abs(a - ar) <= 1e-9 * max(1.0, ar), f"pose case {c}: ADD {a} / {ar}"
    b = reg.ADDS(verts, R[i], t[i], R[j], t[j], surf); br = ro.ADDS(verts.astype(np.float64), R[i], t[i], R[j], t[j], surf.astype(np.float64))
    # f32 winners, exact f64 distances: equal to the KD-tree's except at ties of f32 roundings (1e-7 relative of a distance)
    assert abs(b - br) <= 1e-6 * max(1.0, br), f"pose case {c}: ADD-S {b} / {br}"


def vote_pick_case(c):
    """choosePose.py:98-151 (the n x n ADD-S vote, with and without the distance-field bounds) and verfication.py:61-108 (the
    consecutive-pair Chamfer pick) against the oracle's loops; perturbations sized so that decisions sit near 0.1 x diameter."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import sequence, synth
    from oracle import registration_oracle as ro
    solid = synth.bumpy_ellipsoid if rng.random() < 0.5 else synth.tless_like
    S = solid(rng, int(rng.integers(200, 2500))).astype(np.float32)
    V = solid(rng, int(rng.integers(50, 800))).astype(np.float32)
    diam = synth.diameter(S)
    n = int(rng.integers(2, 9))
    Rg, tg = synth.random_poses(rng, n)
    P = [synth.perturb_pose(rng, Rg[i], tg[i], float(rng.choice([0.5, 3.0, 8.0, 50.0])), float(rng.choice([0.5, 2.0, 0.08 * diam]))) for i in range(n)]
    Rp, tp = np.array([p[0] for p in P]), np.array([p[1] for p in P])
    tag = f"vote / pick case {c}: n={n} |S|={len(S)} |V|={len(V)}"
    rerr, adds = ro.vote(V.astype(np.float64), S.astype(np.float64), ro.rel_pose_table(Rg, tg), ro.rel_pose_table(Rp, tp), diam)
    # an item within 1e-6 mm of the threshold may fall either way (f32 winners against the KD-tree's f64 ones)
    sure = np.abs(adds - 0.1 * diam) > 1e-6
    for bounds in (False, True):
        img, top, err = sequence.vote_choose_image(V, S, Rg, tg, Rp, tp, diam, bounds=bounds)
        assert np.array_equal(err[sure], rerr[sure]), f"{tag}: bounds={bounds}: {int((err != rerr)[sure].sum())} decisions differ"
        if sure.all():
            assert img == int(np.argmax(rerr.sum(1))), f"{tag}: bounds={bounds}: chosen image {img}"
    pts = torch.from_numpy(S).to(dev)
    poses = torch.from_numpy(np.concatenate([Rp, tp[:, :, None]], axis=2).reshape(n, 12)).to(dev)
    idx, val = sequence.pick_by_chamfer(pts, poses, Rg, tg, n)
    Rrel = np.array([ro.calculate_relative_pose(Rg[i], tg[i], Rg[i + 1], tg[i + 1])[0] for i in range(n - 1)])
    ch = ro.chamfer_pairs(S.astype(np.float64), Rp, Rrel)
    assert abs(val - ch.min()) <= 1e-9 * max(1.0, ch.min()) and abs(ch[idx] - ch.min()) <= 1e-9 * max(1.0, ch.min()), \
        f"{tag}: pick {idx} {val} / {int(np.argmin(ch))} {ch.min()}"


def pnp_case(c):
    """The fused PnP + RANSAC pipeline (inference.py:123-134's cv2.solvePnPRansac, restated: oracle/pnp_oracle.py) — hypotheses
    scored, stopping stage, inlier set and refitted pose against the oracle on random problem sizes and outlier fractions."""
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import synth
    from oracle import pnp_oracle as po
    M = int(rng.choice([rng.integers(4, 60), rng.integers(60, 2000), rng.integers(2000, 12000)]))
    H = int(rng.choice([8, 64, 200, 500]))
    conf = float(rng.choice([1.0, 0.99, 0.9]))
    reperr = float(rng.choice([1.0, 2.0, 5.0]))
    sd = int(rng.integers(1 << 30))
    pts = synth.tless_like(rng, 2000)
    Kc = synth.camera()
    R, t = synth.random_poses(rng, 1)
    p3d, p2d, inl = synth.pnp_case(rng, pts, Kc, R[0], t[0], M, float(rng.choice([0.2, 0.5, 1.5])), float(rng.choice([0.0, 0.3, 0.6, 0.85])))
    tag = f"pnp case {c}: M={M} H={H} confidence={conf} reperr={reperr}"
    r = ops.pnp_ransac(torch.from_numpy(p3d).to(dev), torch.from_numpy(p2d).to(dev), Kc, H=H, reperr=reperr, seed=sd, refine_iters=10,
                       confidence=conf)
    o = po.pnp_ransac(p3d, p2d, Kc, H=H, reperr=reperr, seed=sd, refine_iters=10, confidence=conf)
    st = int(r.status.item())
    if int(r.n_eval.item()) == o["n_eval"] and o["best"] == int(np.argmax(o["n_inl"])) if o["best"] >= 0 else True:
        assert st == o["status"], f"{tag}: status {st} / {o['status']}"
    if not o["status"]:
        return
    # the two P3P solvers are independent (device: degenerate conic; oracle: Grunert + Kabsch) and may disagree on marginal
    # triples, which can move the stopping stage and the winner: compared where the oracle's winner is its unique best
    if int(r.n_eval.item()) != o["n_eval"] or o["best"] != int(np.argmax(o["n_inl"])) or st != 1:
        return "skipped"
    if synth.rot_angle(o["Rt_all"][o["best"]][:, :3], R[0]) > 0.2:
        # the winner is not the planted pose (few hypotheses against 85 % outliers: e.g. an object "seen" 18 m away whose 56
        # inliers are chance): the refit of such a set has a flat direction and the two implementations drift apart along it
        return "junk"
    n = int(r.n_inl.item())
    idx = r.inl_idx[:n].cpu().numpy()
    if not np.array_equal(idx, o["inliers"]):
        # a correspondence within 1e-6 px of the threshold under two poses 1e-12 apart may fall either way
        sym = np.setxor1d(idx, o["inliers"])
        pose_ = r.pose.cpu().numpy()
        assert len(sym) <= max(2, M // 2000), (f"{tag}: inlier sets differ in {len(sym)} of {M} ({n} / {len(o['inliers'])}); poses "
                                               f"{synth.rot_angle(pose_[:, :3], o['Rt'][:, :3]):.3g} rad, {np.linalg.norm(pose_[:, 3] - o['Rt'][:, 3]):.3g} mm apart; best "
                                               f"hypothesis {o['best']} with {int(o['n_inl'][o['best']])} inliers of {o['n_eval']} scored; planted inliers {int(inl.sum())}; "
                                               f"t device {pose_[:, 3]}, oracle {o['Rt'][:, 3]}, hypothesis {o['Rt_all'][o['best']][:, 3]}, planted {t[0]}; "
                                               f"hypothesis / planted rotation {synth.rot_angle(o['Rt_all'][o['best']][:, :3], R[0]):.3g} rad")
    pose = r.pose.cpu().numpy()
    same = np.array_equal(idx, o["inliers"])
    if same and not (synth.rot_angle(pose[:, :3], o["Rt"][:, :3]) < 1e-4 and np.linalg.norm(pose[:, 3] - o["Rt"][:, 3]) < 1e-3):
        # A poor winner (few hypotheses, most correspondences outliers: e.g. 71 inliers of 10 924) leaves a refit whose normal
        # equations are ill-conditioned: the two implementations' roundings (fused multiply-adds and a tree sum here, numpy's sums
        # there) move the solution ALONG the valley.  Then the poses must at least be equally good: the same rms reprojection
        # error over the common inlier set, to 1e-6 px.
        X, uv = p3d[idx].astype(np.float64), p2d[idx].astype(np.float64)
        rms = [float(np.sqrt(np.mean(np.sum((po.project(Kc, T[:, :3], T[:, 3], X)[0] - uv) ** 2, axis=1)))) for T in (pose, o["Rt"])]
        assert abs(rms[0] - rms[1]) <= 1e-6, f"{tag}: rms reprojection error {rms[0]:.9f} / {rms[1]:.9f} px over {n} common inliers"
        return "valley"
    assert synth.rot_angle(pose[:, :3], o["Rt"][:, :3]) < 1e-4 and np.linalg.norm(pose[:, 3] - o["Rt"][:, 3]) < 1e-3, \
        (f"{tag}: pose {synth.rot_angle(pose[:, :3], o['Rt'][:, :3]):.3g} rad, {np.linalg.norm(pose[:, 3] - o['Rt'][:, 3]):.3g} mm from the "
         f"oracle's; inlier sets equal {same} ({n} / {len(o['inliers'])}, differing in {len(np.setxor1d(idx, o['inliers']))}); best hypothesis "
         f"{o['best']} with {int(o['n_inl'][o['best']])} inliers of {o['n_eval']} scored; planted inliers {int(inl.sum())}")


def bounds_case(c):
    """isr_adds_bounds: the distance-field brackets of an item's ADD-S sum must contain isr_nn_batched's exact sum — rigid poses,
    poses that are orthonormal only to f32 rounding (pred_R.npy), vertices far off the field's grid."""
    S = rng.normal(0, float(rng.choice([10.0, 40.0])), (int(rng.integers(50, 4000)), 3)).astype(np.float32)
    V = (rng.normal(0, float(rng.choice([10.0, 40.0, 120.0])), (int(rng.integers(1, 1500)), 3))).astype(np.float32)
    B = int(rng.integers(1, 40))
    Tq = np.stack([rand_pose() for _ in range(B)]); Tt = np.stack([rand_pose() for _ in range(B)])
    if rng.random() < 0.5:
        Tt = Tt.astype(np.float32).astype(np.float64)            # orthonormal to f32 only
    if rng.random() < 0.3:
        Tq[:, :, 3] += rng.normal(0, 300.0, (B, 3))                # far off the grid
    fld = ops.dist_field(torch.from_numpy(S).to(dev), cells=int(rng.choice([16, 48, 128])))
    tq, tt = torch.from_numpy(Tq).to(dev), torch.from_numpy(Tt).to(dev)
    lb, ub = ops.adds_bounds(torch.from_numpy(V).to(dev), tq, tt, fld)
    ex = ops.nn_batched(torch.from_numpy(V).to(dev), torch.from_numpy(S).to(dev), tq, tt).sum_d
    lb, ub, ex = lb.cpu().numpy(), ub.cpu().numpy(), ex.cpu().numpy()
    assert np.all(np.isfinite(lb)) and np.all(np.isfinite(ub)) and np.all(lb <= ex) and np.all(ex <= ub), \
        f"bounds case {c}: |S|={len(S)} |V|={len(V)} B={B}: bracket violated by {max((lb - ex).max(), (ex - ub).max()):.3g}"


def batch_cut_case(c):
    """The cut and the assembly for a GROUP of images with ragged device-side counts (isr_select_top_batch, isr_gather_corr_batch;
    inference.py:274-290 per image) and the lse-only call of K1 against the full call's lse."""
    from oracle import registration_oracle as ro
    B, P, N = int(rng.integers(1, 9)), int(rng.choice([rng.integers(1, 40), rng.integers(40, 1200), rng.integers(1200, 9000)])), int(rng.integers(5, 900))
    x = (-rng.exponential(2.0, (B, P))).astype(np.float32)
    if rng.random() < 0.4:
        x = np.round(x * 2) / 2                                  # plateaus
    n = rng.integers(0, P + 1, size=B).astype(np.int32)
    n[rng.integers(B)] = int(rng.choice([0, 1, 2, min(P, 500), min(P, 501), P]))
    idx = rng.integers(N, size=(B, P)).astype(np.int32)
    pts = rng.normal(0, 30, (N, 3)).astype(np.float32)
    pix = (rng.random((B, P, 2)) * 75).astype(np.float32)
    tag = f"batch cut case {c}: B={B} P={P} n={n.tolist()}"
    nd = torch.from_numpy(n).to(dev)
    keep, M, thr = ops.select_top_batch(torch.from_numpy(x).to(dev), n_dev=nd)
    p3d, p2d = ops.gather_corr_batch(torch.from_numpy(idx).to(dev), keep, M, torch.from_numpy(pts).to(dev), torch.from_numpy(pix).to(dev))
    keep, M, p3d, p2d = keep.cpu().numpy(), M.cpu().numpy(), p3d.cpu().numpy(), p2d.cpu().numpy()
    for b in range(B):
        want = ro.filter_top(torch.from_numpy(x[b, : n[b]]).reshape(-1, 1)) if n[b] > 0 else np.zeros(0, np.int64)   # n = 0: IndexError in the reference
        m = int(M[b])
        assert m == len(want) and np.array_equal(keep[b, :m], want), f"{tag}: image {b}: kept {m} / {len(want)}"
        assert np.array_equal(p3d[b, :m], pts[idx[b]][want]) and np.array_equal(p2d[b, :m], pix[b][want]), f"{tag}: image {b}: assembly differs"
    # lse-only K1 call = the full call's lse, bit for bit, on a random route
    D = int(rng.choice([12, 16, 40, 64]))
    Pq, Nk = int(rng.integers(1, 3000)), int(rng.integers(1, 6000))
    Q = rng.normal(0, 1, (Pq, D)).astype(np.float32); K = rng.normal(0, 1, (Nk, D)).astype(np.float32)
    if rng.random() < 0.5:
        q, k, kw = torch.from_numpy(Q).to(dev), torch.from_numpy(K).to(dev), {}
    else:
        q, k, kw = ops.prescale_queries_log2(torch.from_numpy(Q)).to(dev), torch.from_numpy(K).bfloat16().to(dev), dict(log2_prescaled=True)
    full = ops.corr_argmax(q, k, want_lse=True, **kw)[2]
    only = ops.corr_lse(q, k, **kw)
    assert torch.equal(full, only), f"batch cut case {c}: the lse-only call differs from the full call (P={Pq} N={Nk} D={D} {'bf16' if kw else 'f32'})"


worst = 0.0
worst_icp = 0.0
pnp_skipped = pnp_valley = 0
for c in range(cases):
    bounds_case(c)
    batch_cut_case(c)
    rc_ = pnp_case(c)
    pnp_skipped += rc_ in ("skipped", "junk")
    pnp_valley += rc_ == "valley"
    vote_pick_case(c)
    prep_case(c)
    pose_case(c)
    crop_case(c)
    worst = max(worst, corr_case(c))
    nn_case(c)
    ransac_case(c)
    filter_case(c)
    worst_icp = max(worst_icp, icp_case(c))
    if c % 10 == 9:
        print(f"  seed {seed}: {c + 1} cases", flush=True)
print(f"seed {seed}: {cases} corr + {cases} nn + {cases} ransac + {cases} filter + {cases} icp + {cases} crop + {cases} prep + {cases} pose + {cases} vote / pick + {cases} batch cut + {cases} bounds + {cases} pnp cases ok ({pnp_skipped} pnp cases not comparable: the two P3P solvers disagreed on a marginal triple, or the winner is not the planted pose; {pnp_valley} compared by reprojection error: an ill-conditioned refit of a poor winner); worst corr value error {worst:.3g} "
      f"(relative to max(1, |lse|)), worst ICP rotation difference {worst_icp:.3g} rad")
