"""GPU: isr_icp_point_to_point and its _batch twin against the f64 reference of tests/icp_ref.py, pass by pass.

The existing checks compare the END of the loop with the oracle on random surface clouds; the loop is a contracting fixed
point iteration, so a neighbour decided wrongly in one pass is largely forgotten by the next ones, and such clouds hold one
or two near ties per run.  Here the device runs with max_iter = k for k = 0 .. K (LOCKSTEP: K = the reference's stopping
pass + 1, at most 12) and its 20 state doubles — T | fitness, rmse, iterations, correspondences — must equal entry
min(k, last) of the reference's trajectory: iterations and n exactly, fitness to 1e-12, rmse to 1e-9, rotation to 1e-9 rad,
translation to 1e-6 mm (the tolerances of tests/test_gpu_registration.py).  Every case runs as given, with the warm start
off (ops.tuning(icp_warm=0): every pass on the cold kernels), as item 0 of a batch of three (with a second start and a far
one that finds nothing), and — sizes, ties and the tile cull — under the plan knobs that reach the other search
instantiations at small shapes (four queries per lane below 1024 rows, one above; one key range over the whole target, so
that the cold search takes the filter loop).  All of them must agree bit for bit.

The cases (tests/icp_ref.py; tests/test_icp_ref_cpu.py shows that each of them can be compared): sizes at every edge of the
tiling, the stopping rule, lattices on which EVERY point is an exact or a sub-f32 near tie, clouds that exercise the tile
cull, degenerate correspondences for the Horn step, clouds far from the origin.

Sensitivity (tried on scratch builds): with the search's near-tie flag never raised, or with the f64 resolution sweep of
the pass (resolve_flagged, csrc/icp_loop.hpp) dropped, test_lattice_ties[near_tie_pos] and [near_tie_pos_permuted] fail at k = 0; the
one-point-at-the-origin case failed before the near-tie bound returned inf for a best of inf.

Measured agreement: profiles/icp_edges_parity.json (rewritten by running this module with ISR_ICP_EDGES_PARITY_OUT=<file>)."""
import json
import os

import numpy as np
import pytest
import torch

from . import icp_ref as ir

pytestmark = pytest.mark.gpu

TOL = dict(fitness=1e-12, rmse=1e-9, rot=1e-9, trans=1e-6)          # tests/test_gpu_registration.py
MEASURED = {}


def _record(case, k, **kw):
    e = MEASURED.setdefault(case, {}).setdefault(str(k), {})
    for key, v in kw.items():
        e[key] = max(float(v), e.get(key, 0.0))


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    """Writes what the module measured, once it has run, to the file ISR_ICP_EDGES_PARITY_OUT names."""
    yield
    out = os.environ.get("ISR_ICP_EDGES_PARITY_OUT")
    if out:
        what = ("tests/test_gpu_icp_edges.py: per case and per number of updates k the worst difference, over every mode, "
                "between the device's state and the f64 reference of tests/icp_ref.py: rot (rad), trans (mm), rmse (mm), "
                "cloud = largest |T p - T_ref p| over the source (mm)")
        with open(out, "w") as f:
            json.dump({"what": what, "tolerances": TOL, "cases": MEASURED}, f, indent=1)
            f.write("\n")


@pytest.fixture(scope="module")
def reg(cuda0):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import registration
    return registration


@pytest.fixture(scope="module")
def ops(cuda0):
    from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
    return ops


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------- device calls
def single(reg, ops, c, k, init=None, tgt=None, spatial_order=None, **knobs):
    """The 20 state doubles of isr_icp_point_to_point with max_iter = k: registration.icp_point_to_point's own steps (which
    returns three of them), under the tuning knobs given."""
    s = torch.from_numpy(c["src"]).cuda()
    t = torch.from_numpy(np.ascontiguousarray(c["tgt"] if tgt is None else tgt, np.float32)).cuda()
    order = c.get("spatial_order", True) if spatial_order is None else spatial_order
    if order and min(s.shape[0], t.shape[0]) > reg.MORTON_MIN_ROWS:
        s, t = s[reg.morton_order(s)].contiguous(), t[reg.morton_order(t)].contiguous()
    buf = torch.empty(20, dtype=torch.float64, device=s.device)
    T0 = c["init"] if init is None else init
    buf[:16] = torch.from_numpy(np.ascontiguousarray(np.asarray(T0, np.float64).reshape(16))).cuda()
    L = ops.lib()
    with ops.tuning(**knobs):
        ws = ops.workspace(s.device, L.isr_icp_workspace_bytes(s.shape[0], t.shape[0]), "icp")
        rc = L.isr_icp_point_to_point(ops.ptr(s), s.shape[0], ops.ptr(t), t.shape[0], c["threshold"], int(k), c["rel"][0],
                                      c["rel"][1], buf.data_ptr(), buf.data_ptr() + 128, ops.ptr(ws), ws.numel(),
                                      ops.current_stream(s.device))
        ops.check(rc, "isr_icp_point_to_point")
        return buf.cpu().numpy()


def other_starts(c):
    """A second start near the case's, and a far one that finds no correspondence."""
    rng = np.random.default_rng(5)
    far = c["init"].copy()
    far[:3, 3] += 1.0e4
    return np.stack([c["init"], ir.small_pose(rng, 1.0, 0.5) @ c["init"], far])


def batch(reg, c, k, tgt=None, spatial_order=None):
    order = c.get("spatial_order", True) if spatial_order is None else spatial_order
    return reg.icp_batch_state(c["src"], c["tgt"] if tgt is None else tgt, c["threshold"], other_starts(c), max_iter=k,
                               rel_fitness=c["rel"][0], rel_rmse=c["rel"][1], spatial_order=order)


def plan_knobs(c):
    """The other search instantiations at small shapes: four queries per lane below 1024 rows (one above, where four is
    the default); one key range over the whole target — from four tiles on the cold search then takes the filter loop."""
    return [dict(nn_plan_rq=4 if len(c["src"]) < 1024 else 1), dict(nn_plan_blocks=1)]


# ---------------------------------------------------------------------------------------------- comparison
def differences(c, state, e):
    T = state[:16].reshape(4, 4)
    src = c["src"].astype(np.float64)
    return dict(rot=ir.rot_angle(T[:3, :3], e["T"][:3, :3]), trans=float(np.linalg.norm(T[:3, 3] - e["T"][:3, 3])),
                rmse=abs(state[17] - e["rmse"]), fitness=abs(state[16] - e["fitness"]),
                cloud=float(np.abs(ir.transform(T, src) - ir.transform(e["T"], src)).max()))


def against_reference(c, k, state, e, pose=True):
    d = differences(c, state, e)
    _record(c["name"], k, rot=d["rot"], trans=d["trans"], rmse=d["rmse"], cloud=d["cloud"])
    tag = f"{c['name']} k={k}: device {state[16:].tolist()} reference {(e['fitness'], e['rmse'], e['iterations'], e['n'])} {d}"
    assert np.isfinite(state).all() and (state[12:16] == [0, 0, 0, 1]).all(), tag
    assert state[18] == e["iterations"] and state[19] == e["n"], tag
    assert d["fitness"] < TOL["fitness"], tag
    assert d["rmse"] < TOL["rmse"], tag
    if pose:
        assert d["rot"] < TOL["rot"] and d["trans"] < TOL["trans"], tag
    return d


def steps(c, traj):
    last = len(traj) - 1
    K = min(last + 1, 12)
    return range((K if c["kmax"] is None else min(K, c["kmax"])) + 1), last


def all_modes(reg, ops, c, k, knobs=(), tgt=None, spatial_order=None):
    """The state of (c, k) as given — after every other mode has returned the same bits."""
    kw = dict(tgt=tgt, spatial_order=spatial_order)
    base = single(reg, ops, c, k, **kw)
    assert same_bits(single(reg, ops, c, k, icp_warm=0, **kw), base), f"{c['name']} k={k}: warm start off differs"
    for kn in knobs:
        assert same_bits(single(reg, ops, c, k, **kn, **kw), base), f"{c['name']} k={k}: {kn} differs"
        assert same_bits(single(reg, ops, c, k, icp_warm=0, **kn, **kw), base), f"{c['name']} k={k}: {kn}, warm start off differs"
    b = batch(reg, c, k, **kw)
    starts = other_starts(c)
    assert b.shape == (3, 20)
    assert same_bits(b[0], base), f"{c['name']} k={k}: batch item 0 {b[0]} differs from the single call {base}"
    for i in (1, 2):
        assert same_bits(b[i], single(reg, ops, c, k, init=starts[i], **kw)), f"{c['name']} k={k}: batch item {i} differs"
    assert b[2, 19] == 0 and b[2, 18] == 0 and same_bits(b[2, :12], starts[2].reshape(16)[:12])     # the far start found nothing
    return base


def lockstep(reg, ops, c, knobs=(), **kw):
    traj = ir.reference(c["name"])
    ks, last = steps(c, traj)
    out = []
    for k in ks:
        state = all_modes(reg, ops, c, k, knobs)
        against_reference(c, k, state, traj[min(k, last)], **kw)
        out.append(state)
    return out, traj


# ---------------------------------------------------------------------------------------------- (a) sizes
@pytest.mark.parametrize("Ns,Nt", ir.SIZE_PAIRS)
def test_sizes_lockstep(reg, ops, Ns, Nt):
    c = ir.cases()[f"size_{Ns}x{Nt}"]
    states, traj = lockstep(reg, ops, c, plan_knobs(c))
    if Ns < 3:            # never three pairs: T stays the start bit for bit, fitness and rmse are still computed
        for s in states:
            assert same_bits(s[:12], c["init"].reshape(16)[:12]) and s[18] == 0 and s[19] == Ns and s[16] == 1.0 and s[17] > 1.0


@pytest.mark.parametrize("n0", [0, 1, 2, 3])
def test_pass_0_with_0_to_3_correspondences(reg, ops, n0):
    c = ir.cases()[f"count_{n0}"]
    states, traj = lockstep(reg, ops, c, plan_knobs(c))
    assert states[0][19] == n0
    if n0 < 3:
        assert all(same_bits(s[:12], c["init"].reshape(16)[:12]) and s[18] == 0 for s in states)
    else:
        assert states[-1][18] == len(traj) - 1 > 0


def test_one_point_at_the_origin(reg, ops):
    """Ns = Nt = 1, both the origin, T = I: the search's near-tie bound must not turn inf * 0 into a NaN that hides the
    neighbour (fitness 1, rmse 0, one correspondence)."""
    c = ir.cases()["origin_1x1"]
    states, _ = lockstep(reg, ops, c, plan_knobs(c))
    for s in states:
        assert s[16:].tolist() == [1.0, 0.0, 0.0, 1.0] and same_bits(s[:16], np.eye(4).reshape(16))


# ---------------------------------------------------------------------------------------------- (b) the stopping rule
def test_max_iter_0(reg, ops):
    c = ir.cases()["size_257x513"]
    s = all_modes(reg, ops, c, 0)
    against_reference(c, 0, s, ir.reference(c["name"])[0])
    assert s[18] == 0 and s[19] > 3 and same_bits(s[:12], c["init"].reshape(16)[:12])


def test_source_equal_to_target_stops_after_one_update(reg, ops):
    c = ir.cases()["source_is_target"]
    states, traj = lockstep(reg, ops, c)
    assert len(states) == 3 and [s[18] for s in states] == [0, 1, 1]
    assert states[0][17] == 0.0 and states[0][16] == 1.0


def test_zero_tolerances_never_converge(reg, ops):
    c = ir.cases()["rel_zero"]
    states, traj = lockstep(reg, ops, c)
    assert [s[18] for s in states] == list(range(13))
    # the loop does not stop short of its budget later on either (no reference beyond 12 updates: the count alone)
    assert single(reg, ops, c, 40)[18] == 40


@pytest.mark.parametrize("inside", [True, False])
def test_radius_boundary(reg, ops, inside):
    """Every distance exactly 5 on integer coordinates: threshold 5.0 counts every pair, the double below it none."""
    c = ir.cases()["radius_5_in" if inside else "radius_5_out"]
    states, traj = lockstep(reg, ops, c)
    if inside:
        assert states[0][16:].tolist() == [1.0, 5.0, 0.0, 100.0] and states[-1][18] == 2
    else:
        assert all(s[16:].tolist() == [0.0, 0.0, 0.0, 0.0] and same_bits(s[:16], np.eye(4).reshape(16)) for s in states)


# ---------------------------------------------------------------------------------------------- (c) ties
@pytest.mark.parametrize("name", ["near_tie_pos", "near_tie_neg", "near_tie_pos_permuted", "exact_tie"])
def test_lattice_ties(reg, ops, name):
    """Every source point has eight targets at one f32 distance.  near_tie: f64 tells them apart by a relative 1.3e-9 and
    the winner has the HIGHEST index of the eight (pos); exact_tie: the lowest index wins.  An f32 search alone moves the
    cloud by (-1, -1, -1) in every one of them."""
    c = ir.cases()[name]
    states, traj = lockstep(reg, ops, c, plan_knobs(c))
    assert states[0][19] == 125
    assert np.abs(states[1][:16].reshape(4, 4) - ir.pose(t=c["step"])).max() < 1e-9, states[1]


@pytest.mark.parametrize("Ns,spatial_order", [(255, True), (257, False), (257, True)])
def test_every_point_flagged_every_pass(reg, ops, Ns, spatial_order):
    """The target twice over: every source point has two targets at the same distance, 700 rows — several key ranges —
    apart, in every pass (Ns is no multiple of the resolution sweep's four).  Only the index may differ from the run against
    the target itself: the 20 doubles are the same bits."""
    c = ir.cases()[f"duplicates_{Ns}"]
    traj = ir.reference(c["name"])
    ks, last = steps(c, traj)
    for k in ks:
        s1 = all_modes(reg, ops, c, k, plan_knobs(c), spatial_order=spatial_order)
        s2 = all_modes(reg, ops, c, k, plan_knobs(c), tgt=c["tgt2"], spatial_order=spatial_order)
        assert same_bits(s1, s2), f"{c['name']} k={k}: {s2} against the doubled target, {s1} against the target"
        against_reference(c, k, s2, traj[min(k, last)])


# ---------------------------------------------------------------------------------------------- (d) the tile cull
@pytest.mark.parametrize("kind", ir.CULL_KINDS)
def test_tile_cull(reg, ops, kind):
    """Under the plan knobs too: one query per lane and four (a workgroup of 256 rows or of 1024 against the tile boxes),
    one-tile key ranges (a workgroup whose every wave culls its tile leaves without posting) and one range over all tiles
    (the waves skip tile by tile)."""
    c = ir.cases()[f"cull_{kind}"]
    states, traj = lockstep(reg, ops, c, plan_knobs(c))
    if kind == "far_rows":          # the condition on the case: its first 256 rows never count, the loop goes on without them
        assert len(c["src"]) == 1023 and all(s[19] == 1023 - 256 for s in states) and states[-1][18] >= 3


# ---------------------------------------------------------------------------------------------- (e) geometry of the update
@pytest.mark.parametrize("kind", ir.GEOMETRY_KINDS + ["volume"])
def test_update_geometry(reg, ops, kind):
    """One update on coplanar pairs, on a slab against its mirror image (Kabsch's d = -1 branch), on exactly three pairs."""
    c = ir.cases()[f"geometry_{kind}"]
    states, traj = lockstep(reg, ops, c)
    R = states[1][:16].reshape(4, 4)[:3, :3]
    assert abs(np.linalg.det(R) - 1) < 1e-14 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14


@pytest.mark.parametrize("name", ["collinear", "one_target"])
def test_update_without_a_unique_rotation(reg, ops, name):
    """Collinear pairs, and every point matched to one target (S = 0): only what the reference defines — a finite, proper
    rigid step whose residual over the pass-0 pairs is the Kabsch optimum; for S = 0 that is the identity rotation."""
    c = ir.cases()[name]
    traj = ir.reference(name)
    s0 = all_modes(reg, ops, c, 0)
    against_reference(c, 0, s0, traj[0])
    s1 = all_modes(reg, ops, c, 1)
    T = s1[:16].reshape(4, 4)
    R = T[:3, :3]
    assert np.isfinite(s1).all() and s1[18] == 1
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
    P, Q = traj[0]["P"], traj[0]["Q"]                           # (the start is the identity: T is the step itself)
    best = ir.residual(ir.kabsch(P, Q), P, Q)
    got = ir.residual(T, P, Q)
    print(f"{name}: residual {got!r}, Kabsch optimum {best!r}, rotation {ir.rot_angle(R, np.eye(3)):.3e} rad off the identity")
    _record(name, 1, residual_rel=abs(got - best) / best)
    assert abs(got - best) <= 1e-9 * best
    if name == "one_target":
        assert np.array_equal(R, np.eye(3))
        assert abs(got - ir.residual(ir.pose(t=Q.mean(0) - P.mean(0)), P, Q)) <= 1e-9 * best


# ---------------------------------------------------------------------------------------------- (f) distance from the origin
@pytest.mark.parametrize("offset", ir.OFFSETS)
def test_one_update_far_from_the_origin(reg, ops, offset):
    """The covariance is formed from uncentred f64 sums: the pose tolerances are asserted at 700 mm (the working distance),
    1e-6 mm at the cloud and the rmse at every offset; the pose differences beyond are recorded
    (profiles/icp_edges_parity.json)."""
    c = ir.cases()[f"offset_{int(offset)}"]
    states, traj = lockstep(reg, ops, c, pose=offset <= 700.0)
    for k, s in enumerate(states):
        d = differences(c, s, traj[k])
        print(f"offset {offset}: k={k} {d}")
        assert d["cloud"] < 1e-6, (offset, k, d)


def test_lockstep_at_700_mm(reg, ops):
    lockstep(reg, ops, ir.cases()["offset_700_lockstep"])
