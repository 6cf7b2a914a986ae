"""CPU: the host build of the fused Adam (isr_adam_step_host, compiled from csrc/adam.hpp like the kernel) against
tests/adam_ref.py bit for bit over the size edges, the paired powering against math.pow, the ramp against trainPose.py's
expression, the accuracy against torch.optim.Adam in f64 with torch's own f32 Adam as the yardstick, and the edge inputs."""
import ctypes
import math

import numpy as np
import pytest
import torch

from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops

from . import adam_ref as ref

f32, f64 = np.float32, np.float64
#          lr,   beta1, beta2, eps,  weight_decay, ramp
PLAIN = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
RAMPED = (3e-4, 0.9, 0.999, 1e-8, 0.01, 2000.0)


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_geometry_matches_the_binding(hip_lib):
    g = ops.adam_geometry()
    assert g == {"tensor_bytes": ops.ADAM_TENSOR.itemsize, "chunk": ops.ADAM_CHUNK, "threads": 256, "max_groups": ops.ADAM_MAX_GROUPS}
    assert ref.CHUNK == g["chunk"] and g["tensor_bytes"] == 48


def test_host_bits_equal_numpy_over_the_size_edges(hip_lib):
    """Every element count of ref.SIZES twice (one tensor per group), three steps from counters 0, 1 and 1998 (so the ramp
    crosses its end), views at every misalignment."""
    sizes = list(ref.SIZES) * 2
    T = len(sizes)
    group_of = [i % 2 for i in range(T)]
    offsets = [i % 4 for i in range(T)]
    mine = ref.make_tensors(sizes, seed=1, offsets=offsets)
    theirs = ref.clone(mine)
    steps_a = np.array([(0, 1, 1998)[i % 3] for i in range(T)], np.int64)
    steps_b = steps_a.copy()
    rng = np.random.default_rng(2)
    for it in range(3):
        ops.adam_step_host(*mine, group_of, [PLAIN, RAMPED], steps_a)
        ref.step(*theirs, group_of, [PLAIN, RAMPED], steps_b)
        for k, name in enumerate("pgmv"):
            for i in range(T):
                assert ref.same_bits(mine[k][i], theirs[k][i]), (it, name, i, sizes[i])
        assert np.array_equal(steps_a, steps_b)
        for i in range(T):                                                            # new gradients for the next step
            mine[1][i][...] = theirs[1][i][...] = (mine[1][i] * rng.uniform(0.5, 1.5, sizes[i])).astype(f32)
    assert steps_a.tolist() == [(3, 4, 2001)[i % 3] for i in range(T)]


def test_slots_and_zero_grads(hip_lib):
    """Tensors pointing at scattered counters; zero_grads stores +0 and changes nothing else."""
    sizes = [65, ref.CHUNK + 1, 0, 5]
    a = ref.make_tensors(sizes, seed=3)
    b = ref.clone(a)
    sa, sb = np.array([7, 0, 0, 3, 0, 11], np.int64), np.array([7, 0, 0, 3, 0, 11], np.int64)
    slots = [5, 0, 3, 2]
    ops.adam_step_host(*a, [0, 1, 1, 0], [PLAIN, RAMPED], sa, slots=slots, zero_grads=True)
    ops.adam_step_host(*b, [0, 1, 1, 0], [PLAIN, RAMPED], sb, slots=slots, zero_grads=False)
    assert sa.tolist() == sb.tolist() == [8, 0, 1, 4, 0, 12]
    for k in (0, 2, 3):
        assert all(ref.same_bits(x, y) for x, y in zip(a[k], b[k]))
    assert all(np.array_equal(ref.bits(g), np.zeros(g.size, np.uint32)) for g in a[1])      # +0, not -0
    assert all(np.any(g != 0) for g in b[1] if g.size)


@pytest.mark.parametrize("beta", [0.9, 0.999])
@pytest.mark.parametrize("t", [1, 2, 3, 1999, 2000, 2001, 10 ** 6])
def test_powering_within_4_ulp_of_pow(hip_lib, beta, t):
    got = ops.adam_scalars_host((1e-3, beta, beta, 1e-8, 0.0, 0.0), t)
    want = math.pow(beta, t)
    assert got["beta1_t"] == got["beta2_t"] == ref.pow_int(beta, t)                   # the host build is the stated recipe
    ulps = abs(got["beta1_t"] - want) / math.ulp(want) if want != got["beta1_t"] else 0.0
    print(f"beta {beta} t {t}: {ulps} ulp from math.pow")
    assert ulps <= 4


@pytest.mark.parametrize("t", [1, 2, 3, 1999, 2000, 2001, 10 ** 6])
def test_powering_is_exact_for_one_half(hip_lib, t):
    got = ops.adam_scalars_host((1e-3, 0.5, 0.5, 1e-8, 0.0, 0.0), t)["beta1_t"]
    assert got == (math.ldexp(1.0, -t) if t <= 1074 else 0.0)


@pytest.mark.parametrize("lr", [3e-5, 3e-4])
def test_ramp_is_trainpose_expression(hip_lib, lr):
    for t in (1, 1998, 1999, 2000):
        frac = (t + 1) / 2000                                                         # trainPose.py:230-232, iteration = t
        if frac >= 1:
            frac = 1
        assert ops.adam_scalars_host((lr, 0.9, 0.999, 1e-8, 0.0, 2000.0), t)["lr_t"] == lr * frac == ref.lr_at(lr, 2000.0, t)
        assert ops.adam_scalars_host((lr, 0.9, 0.999, 1e-8, 0.0, 0.0), t)["lr_t"] == lr
    assert ops.adam_scalars_host((lr, 0.9, 0.999, 1e-8, 0.0, 2000.0), 1998)["lr_t"] < lr
    assert ops.adam_scalars_host((lr, 0.9, 0.999, 1e-8, 0.0, 2000.0), 1999)["lr_t"] == lr


def test_scalars_are_the_reference_scalars(hip_lib):
    for group in (PLAIN, RAMPED):
        for t in (1, 2, 7, 1999, 2000, 123456):
            got = ops.adam_scalars_host(group, t)
            step, r = ref.scalars(group, t)
            assert got["step"].tobytes() == step.tobytes() and got["r"].tobytes() == r.tobytes()


def torch_adam_run(dtype, group, p0, grads, steps):
    """torch.optim.Adam on the CPU, the ramp applied through param_groups as trainPose.py:229-236 does -> the parameters."""
    lr, b1, b2, eps, wd, ramp = group
    ps = [torch.nn.Parameter(torch.from_numpy(p.astype(f64)).to(dtype)) for p in p0]
    opt = torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for it in range(steps):
        iteration = it + 1
        if ramp > 0:
            frac = (iteration + 1) / ramp
            for pg in opt.param_groups:
                pg["lr"] = lr * (1 if frac >= 1 else frac)
        for p, g in zip(ps, grads[it]):
            p.grad = torch.from_numpy(g.astype(f64)).to(dtype)
        opt.step()
    return [p.detach().numpy().astype(f64) for p in ps]


ACCURACY_SIZES = (65, ref.CHUNK + 1)
ACCURACY_STEPS = 30


def accuracy_inputs():
    p, _, _, _ = ref.make_tensors(ACCURACY_SIZES, seed=11)
    grads = [ref.make_tensors(ACCURACY_SIZES, seed=100 + it)[1] for it in range(ACCURACY_STEPS)]      # 1e-6 .. 10, either sign
    return p, grads


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("lr,ramp", [(1e-3, 0.0), (3e-4, 2000.0)])
def test_accuracy_against_torch_f64(hip_lib, lr, ramp, wd):
    """30 steps; the largest |p - p64| of the host build may be at most twice torch-f32's own: both are f32 roundings of one
    formula in different orders."""
    group = (lr, 0.9, 0.999, 1e-8, wd, ramp)
    p0, grads = accuracy_inputs()
    p64 = torch_adam_run(torch.float64, group, p0, grads, ACCURACY_STEPS)
    p32 = torch_adam_run(torch.float32, group, p0, grads, ACCURACY_STEPS)
    p = [a.copy() for a in p0]
    m, v = [np.zeros_like(a) for a in p0], [np.zeros_like(a) for a in p0]
    steps = np.zeros(len(p), np.int64)
    for it in range(ACCURACY_STEPS):
        ops.adam_step_host(p, [g.copy() for g in grads[it]], m, v, [0] * len(p), [group], steps)
    ours = max(float(np.abs(a.astype(f64) - b).max()) for a, b in zip(p, p64))
    theirs = max(float(np.abs(a - b).max()) for a, b in zip(p32, p64))
    moved = max(float(np.abs(a.astype(f64) - b).max()) for a, b in zip(p0, p64))
    print(f"lr {lr} ramp {ramp} wd {wd}: host build {ours:.3e}, torch f32 {theirs:.3e}, the parameters moved {moved:.3e}")
    assert moved > 100 * theirs and theirs > 0
    assert ours <= 2 * theirs


def test_zero_gradients_give_eps_as_denominator(hip_lib):
    """g = 0 throughout: v stays 0, the denominator is eps, and m = 0 gives p' = p exactly; with m != 0, p' = p - step m' / eps."""
    n = 70
    p, _, m, _ = ref.make_tensors([n], seed=5)
    g, v = [np.zeros(n, f32)], [np.zeros(n, f32)]
    p0, m0 = p[0].copy(), m[0].copy()
    steps = np.zeros(1, np.int64)
    ops.adam_step_host(p, g, m, v, [0], [PLAIN], steps)
    assert np.all(v[0] == 0)
    step, r = ref.scalars(PLAIN, 1)
    m1 = ref.fmaf(f32(1.0 - 0.9), (g[0] - m0).astype(f32), m0)
    want = ref.fmaf(-step, (m1 / f32(1e-8)).astype(f32), p0)                          # sqrt(0) / r + eps = eps
    assert ref.same_bits(p[0], want) and ref.same_bits(m[0], m1)
    z = [np.zeros(n, f32)]
    ops.adam_step_host(p, g, z, v, [0], [PLAIN], steps)                               # m = 0 too: nothing moves
    assert ref.same_bits(p[0], want) and np.all(z[0] == 0)


def test_non_finite_gradients_propagate_as_in_the_reference(hip_lib):
    sizes = [9, 65]
    a = ref.make_tensors(sizes, seed=6)
    for g in a[1]:
        g[0], g[1], g[2], g[4] = np.inf, -np.inf, np.nan, f32(3e38)                   # 3e38 squared overflows
    b = ref.clone(a)
    sa, sb = np.zeros(2, np.int64), np.zeros(2, np.int64)
    for _ in range(2):
        ops.adam_step_host(*a, [0, 1], [PLAIN, RAMPED], sa)
        ref.step(*b, [0, 1], [PLAIN, RAMPED], sb)
    for k in range(4):
        assert all(ref.same_bits(x, y) for x, y in zip(a[k], b[k]))
    assert all(np.isnan(p[:3]).all() and np.isfinite(p[5:]).all() for p in a[0])


def _raw_table(arrays, n, group=0, slot=0):
    t = np.zeros(1, ops.ADAM_TENSOR)
    t[0] = (*[a.ctypes.data for a in arrays], n, group, slot)
    return t


BAD_GROUPS = {
    "lr < 0": (-1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0), "beta1 = 1": (1e-3, 1.0, 0.999, 1e-8, 0.0, 0.0),
    "beta2 < 0": (1e-3, 0.9, -0.1, 1e-8, 0.0, 0.0), "eps = 0": (1e-3, 0.9, 0.999, 0.0, 0.0, 0.0),
    "weight_decay < 0": (1e-3, 0.9, 0.999, 1e-8, -0.1, 0.0), "ramp < 0": (1e-3, 0.9, 0.999, 1e-8, 0.0, -1.0),
    "lr NaN": (float("nan"), 0.9, 0.999, 1e-8, 0.0, 0.0), "eps inf": (1e-3, 0.9, 0.999, float("inf"), 0.0, 0.0),
}


def test_bad_arguments_are_refused_and_nothing_is_written(hip_lib):
    L = hip_lib
    arrays = [np.full(8, x, f32) for x in (1.0, 2.0, 3.0, 4.0)]
    before = [a.copy() for a in arrays]
    steps = np.array([5], np.int64)
    ok = np.asarray([PLAIN], f64)

    def refused(table, T, groups, G, n_slots=1, frag=b""):
        rc = L.isr_adam_step_host(_hp(table), T, _hp(groups), G, _hp(steps), n_slots, 1)
        assert rc == -1 and frag in L.isr_last_error(), (rc, L.isr_last_error())
        assert steps[0] == 5 and all(np.array_equal(a, b) for a, b in zip(arrays, before))

    good = _raw_table(arrays, 8)
    for what, g in BAD_GROUPS.items():
        refused(good, 1, np.asarray([g], f64), 1, frag=b"group 0")
    refused(good, 1, ok, 0, frag=b"G=0")
    refused(good, 1, np.repeat(ok, 9, 0), 9, frag=b"G=9")
    refused(good, -1, ok, 1, frag=b"T=-1")
    refused(_raw_table(arrays, -1), 1, ok, 1, frag=b"negative element count")
    refused(_raw_table(arrays, 8, group=1), 1, ok, 1, frag=b"group index")
    refused(_raw_table(arrays, 8, slot=1), 1, ok, 1, frag=b"step slot")
    two = np.concatenate([good, _raw_table([np.zeros(8, f32) for _ in range(4)], 8)])
    refused(two, 2, ok, 1, frag=b"share a step slot")
    odd = _raw_table(arrays, 4)
    odd["g"][0] += 2
    refused(odd, 1, ok, 1, frag=b"4-byte aligned")
    null = _raw_table(arrays, 8)
    null["v"][0] = 0
    refused(null, 1, ok, 1, frag=b"null array")
    # the device entries check what they can see before any launch: no device is needed for a refusal
    assert L.isr_adam_step(None, None, 1, 1, _hp(ok), 1, None, 0, None) == -1 and b"null table" in L.isr_last_error()
    assert L.isr_adam_step(None, None, 0, 0, _hp(np.asarray([BAD_GROUPS["eps = 0"]], f64)), 1, None, 0, None) == -1
    assert L.isr_adam_zero_grads(None, None, -1, 0, None) == -1
    assert L.isr_adam_scalars_host(_hp(ok), 0, _hp(np.zeros(4)), _hp(np.zeros(2, f32))) == -1
    # T = 0 is a no-op
    assert L.isr_adam_step_host(None, 0, _hp(ok), 1, None, 0, 0) == 0
    assert L.isr_adam_step(None, None, 0, 0, _hp(ok), 1, None, 0, None) == 0
    assert L.isr_adam_zero_grads(None, None, 0, 0, None) == 0


def test_table_check_and_chunk_starts(hip_lib):
    sizes = list(ref.SIZES)
    arrays = ref.make_tensors(sizes, seed=8)
    table = np.zeros(len(sizes), ops.ADAM_TENSOR)
    for i, n in enumerate(sizes):
        table[i] = (*[arrays[k][i].ctypes.data for k in range(4)], n, i % 2, i)
    chunk_start, chunks = ops.adam_table_host(table, 2, len(sizes))
    want = np.concatenate([[0], np.cumsum([(n + ref.CHUNK - 1) // ref.CHUNK for n in sizes])])
    assert chunk_start.tolist() == want.tolist() and chunks == want[-1] == 0 + 7 + 1 + 1 + 2 + 3
    empty, none = ops.adam_table_host(np.zeros(0, ops.ADAM_TENSOR), 1, 0)
    assert empty.tolist() == [0] and none == 0
    table["slot"][3] = table["slot"][2]
    with pytest.raises(Exception, match="share a step slot"):
        ops.adam_table_host(table, 2, len(sizes))
