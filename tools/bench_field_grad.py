"""The trainable key field (fields.TrainableKeyField: isr_field_pack_device + isr_field_eval forward, isr_field_backward
backward), forward plus backward for the reference's head (3, 256, 256, 256, 12), timed with HIP events:
    python tools/bench_field_grad.py [--out profiles/field_grad.json] [--rounds 7] [--calls 10]
  * run A, trainPose.py's shape: 32 768 points (16 x 1 024 positives and as many negatives);
  * run B: 1 024 points.
Each against
  * the same weights as tests/field_ref.py's TorchField under torch autograd on the same device and inputs, in 16 chunks as
    the reference's batched_customForward chunks them;
  * the launch floor: as many one-element fills as the route launches kernels (the pack, the forward, and of the backward one per
    slab and two per batch), what those launches cost whatever they compute;
  * the f32 matrix peak (157.3 TFLOP/s): the forward, its recomputation, the u pass and the dW pass counted as issued FLOPs
    (ops.field_flops + ops.field_backward_flops).
Peak memory (torch.cuda.max_memory_allocated beyond what was allocated before the call, the inputs and the gradients
subtracted) of both routes goes into the same record.  A round is `calls` forward+backward calls between two events, after one
warm-up call of every route; the record holds the median, the fastest and the slowest round per call.  The gradients are compared
with torch's before timing.  No threshold: the record is the measurement."""
import argparse, ctypes, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import TrainableKeyField
from tests import field_ref

WIDTHS, OMEGAS = (3, 256, 256, 256, 12), (30.0, 30.0, 30.0, 30.0)
F32_MATRIX_PEAK = 157.3e12


def timed(fn, rounds, calls):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "rounds": rounds,
            "calls_per_round": calls}


def peak(fn, dev, release):
    release()                       # the previous call's gradients and the cached workspace: the peak counts them afresh
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def case(name, N, dev, rounds, calls):
    Ws, bs = field_ref.siren_params(WIDTHS, OMEGAS, seed=1)
    rng = np.random.default_rng(2)
    pts = torch.from_numpy(rng.uniform(-1, 1, (N, 3)).astype(np.float32)).to(dev)
    up = torch.from_numpy(rng.standard_normal((N, WIDTHS[-1])).astype(np.float32)).to(dev)
    field = TrainableKeyField(Ws, bs, OMEGAS, dev)
    ref = field_ref.TorchField(Ws, bs, OMEGAS).to(dev)

    def fused():
        field.zero_grad(set_to_none=True)
        field(pts).backward(up)

    def reference():
        ref.zero_grad(set_to_none=True)
        outs = []
        for x in torch.chunk(pts, 16):
            for m, om in zip(ref.linears, ref.omegas):
                x = torch.sin(om * m(x)) if om is not None else m(x)
            outs.append(x)
        torch.cat(outs).backward(up)

    fused()
    reference()
    rel = {}
    for l, (w, b, m) in enumerate(zip(field.weights, field.biases, ref.linears)):
        rel[f"dW_{l}"] = float((w.grad - m.weight.grad).abs().max() / m.weight.grad.abs().max())
        rel[f"db_{l}"] = float((b.grad - m.bias.grad).abs().max() / m.bias.grad.abs().max())
    geo = ops.field_grad_geometry()
    slab = geo["slab"]
    launches = 2 + sum(1 + 2 * -(-min(slab, N - s0) // geo["batch"]) for s0 in range(0, N, slab))
    one = torch.empty(1, dtype=torch.int32, device=dev)
    flop = N * (ops.field_flops(WIDTHS) + ops.field_backward_flops(WIDTHS))
    grads = 4 * sum(ops.field_param_sizes(WIDTHS))
    rec = {"case": name, "N": N, "widths": list(WIDTHS), "kernel_launches": launches, "slabs": (N + slab - 1) // slab,
           "largest_gradient_difference_from_torch_relative_to_the_largest_gradient": rel}
    rec["fused_events"] = timed(fused, rounds, calls)
    rec["torch_events"] = timed(reference, rounds, max(calls // 2, 2))
    rec["launch_floor_fills_events"] = timed(lambda: [one.fill_(1) for _ in range(launches)], rounds, calls)
    rec["fused_events_again"] = timed(fused, rounds, calls)
    rec["issued_flop"] = flop
    rec["f32_matrix_peak_floor_ms"] = round(flop / F32_MATRIX_PEAK * 1e3, 4)
    def release():
        field.zero_grad(set_to_none=True)
        ref.zero_grad(set_to_none=True)
        field._packed = None
        ops.clear_workspaces()

    rec["fused_peak_bytes_beyond_inputs_and_gradients"] = peak(fused, dev, release) - grads
    rec["torch_peak_bytes_beyond_inputs_and_gradients"] = peak(reference, dev, release) - grads
    rec["fused_workspace_bytes"] = int(ops.lib().isr_field_grad_workspace_bytes(len(WIDTHS) - 1, (ctypes.c_int32 * len(WIDTHS))(*WIDTHS), N))
    ms = rec["fused_events"]["median_ms"]
    rec["torch_over_fused"] = round(rec["torch_events"]["median_ms"] / ms, 3)
    rec["fused_over_launch_floor"] = round(ms / rec["launch_floor_fills_events"]["median_ms"], 2)
    rec["fused_over_f32_matrix_peak_floor"] = round(ms / rec["f32_matrix_peak_floor_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    rows = [case("A: trainPose.py's keys, 16 x 1 024 positives and as many negatives", 32768, dev, a.rounds, a.calls),
            case("B: 1 024 points", 1024, dev, a.rounds, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "TrainableKeyField(points).backward(upstream) against the same layers as torch.nn.Linear modules under torch "
                               "autograd on the same device and inputs in 16 chunks, the launch floor (one-element fills, one per kernel "
                               "launch of the fused route) and the f32 matrix peak over the issued FLOPs (forward, recomputation, u pass, "
                               "dW pass).  HIP events around `calls_per_round` forward+backward calls, per call; one process; peak bytes "
                               "beyond what was allocated before the call, minus the gradients",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "the kernels apart (pack, forward, tile, dW, combine); hardware counters (MFMA utilisation, LDS bank "
                                       "conflicts, HBM traffic of the block sums); widths other than the reference's head; the step inside "
                                       "trainPose.py (its UNet is a torch module)",
                       "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
