"""The trainable radiance field (fields.TrainableRadianceField: isr_radiance_pack_device + isr_radiance_render forward,
isr_radiance_backward backward), forward plus backward for the reference's net (H 60, 256-256, Wc 256, C 3) at
trainNerfFine.py's shapes, timed with HIP events:
    python tools/bench_radiance_grad.py [--out profiles/radiance_grad.json] [--rounds 5] [--calls 4]
  * run A: 1 200 rays x 64 samples (the coarse pass);  run B: 1 200 rays x 128 samples (the fine pass).
Each against
  * the same layers as a torch module (tests/radiance_grad_ref.py's TorchRadianceGrad) under torch autograd on the same
    device and inputs, in 16 chunks of rays as the reference's batched_forward chunks them;
  * the launch floor: as many one-element fills as the route launches kernels (the pack, the two of the forward, and of the
    backward two per slab and two per batch), what those launches cost whatever they compute;
  * the f32 matrix peak (157.3 TFLOP/s): the forward, its recomputation, the u pass and the dW pass counted as issued FLOPs
    (ops.radiance_flops + ops.radiance_backward_flops).
Peak memory (torch.cuda.max_memory_allocated beyond what was allocated before the call, the gradients subtracted) of both
routes goes into the same record, and whether two calls of the fused route give identical bytes.  A round is `calls`
forward+backward calls between two events, after one warm-up call of every route; the record holds the median, the fastest
and the slowest round per call.  No threshold: the record is the measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import TrainableRadianceField
from tests import density_ref as dr, radiance_grad_ref as gr, radiance_ref as rr

NAME = gr.REFERENCE
F32_MATRIX_PEAK = 157.3e12


class Bundle:
    def __init__(self, o, d, ln):
        self.origins, self.directions, self.lengths = o, d, ln


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


def case(name, N, P, dev, rounds, calls):
    H, widths, Wc, C = gr.FIELDS[NAME]
    w = gr.weights(NAME)
    o, d, ln = (torch.from_numpy(a).to(dev) for a in rr.bundle(N, P))
    dd, dc = (torch.from_numpy(a).to(dev) for a in gr.upstream(N, P, C))
    field = TrainableRadianceField(*w, dr.frequencies(H), gr.BETA, dev)
    ref = gr.TorchRadianceGrad(w, dr.frequencies(H), gr.BETA).to(dev)
    bundle = Bundle(o, d, ln)

    def fused():
        field.zero_grad(set_to_none=True)
        dens, col = field(bundle)
        torch.autograd.backward([dens, col], [dd[..., None], dc])

    unit = torch.from_numpy(rr.normalize_host(d.cpu().numpy())).to(dev)

    def reference(same_unit_vectors=False):
        ref.zero_grad(set_to_none=True)
        for oc, dn, lc, ddc, dcc, uc in zip(*(torch.chunk(a, 16) for a in (o, d, ln, dd, dc, unit))):
            dens, col = ref(oc, dn, lc, unit_dirs=uc if same_unit_vectors else None)
            torch.autograd.backward([dens, col], [ddc[..., None], dcc])

    fused()
    first = [p.grad.clone() for p in field.parameters()]
    fused()
    identical = all(torch.equal(a.view(torch.int32), p.grad.view(torch.int32)) for a, p in zip(first, field.parameters()))
    # the comparison runs on the library's unit vectors: torch's own normalize on the device may differ in the last bit, which
    # at H = 60 is another direction embedding; the timed route below uses torch's own
    reference(same_unit_vectors=True)
    lins = [x for x in ref.mlp if isinstance(x, torch.nn.Linear)] + [ref.density_layer[0], ref.color_layer[0], ref.color_layer[2]]
    mine = list(zip([*field.weights, *field.color_weights], [*field.biases, *field.color_biases]))
    rel = {}
    for l, ((wp, bp), m) in enumerate(zip(mine, lins)):
        rel[f"dW_{l}"] = float((wp.grad - m.weight.grad).abs().max() / m.weight.grad.abs().max())
        rel[f"db_{l}"] = float((bp.grad - m.bias.grad).abs().max() / m.bias.grad.abs().max())
    geo = ops.radiance_grad_geometry()
    slab, points = geo["slab"], N * P
    launches = 3 + sum(2 + 2 * -(-min(slab, points - s0) // geo["batch"]) for s0 in range(0, points, slab))
    one = torch.empty(1, dtype=torch.int32, device=dev)
    flop = points * (ops.radiance_flops(widths, H, Wc, C) + ops.radiance_backward_flops(widths, H, Wc, C))
    grads = 4 * sum(ops.radiance_param_sizes(widths, H, Wc, C))
    rec = {"case": name, "rays": N, "samples": P, "points": points, "net": NAME, "kernel_launches": launches,
           "slabs": (points + slab - 1) // slab, "two_calls_identical_bytes": bool(identical),
           "largest_gradient_difference_from_torch_f32_relative_to_the_largest_gradient": rel}
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
    ms = rec["fused_events"]["median_ms"]
    rec["torch_over_fused"] = round(rec["torch_events"]["median_ms"] / ms, 3)
    rec["fused_over_launch_floor"] = round(ms / rec["launch_floor_fills_events"]["median_ms"], 2)
    rec["fused_over_f32_matrix_peak_floor"] = round(ms / rec["f32_matrix_peak_floor_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    rows = [case("A: trainNerfFine.py's coarse pass, 1 200 rays x 64 samples", 1200, 64, dev, a.rounds, a.calls),
            case("B: its fine pass, 1 200 rays x 128 samples", 1200, 128, dev, a.rounds, a.calls)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "TrainableRadianceField(bundle) forward + backward against the same layers as a torch module under torch "
                               "autograd on the same device and inputs in 16 chunks of rays, the launch floor (one-element fills, one per "
                               "kernel launch of the fused route) and the f32 matrix peak over the issued FLOPs (forward, recomputation, u "
                               "pass, dW pass).  HIP events around `calls_per_round` forward+backward calls, per call; one process; peak "
                               "bytes beyond what was allocated before the call, minus the gradients",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "the kernels apart (pack, direction terms, render, tile, dW, combine); hardware counters (MFMA "
                                       "utilisation, LDS bank conflicts, HBM traffic of the slab and the block sums); other slab and batch "
                                       "sizes; nets other than the reference's; the whole of training.nerf_train_step",
                       "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
