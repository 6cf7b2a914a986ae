"""The contrastive key loss (losses.contrastive_loss: isr_contrastive_forward + isr_contrastive_backward), forward plus
backward, timed with HIP events:
    python tools/bench_contrastive.py [--out profiles/contrastive.json] [--rounds 7] [--calls 10]
  * trainPose.py's own shape: B = 16, S = 1 024, M = 1 024 negatives per batch item, D = 12;
  * the shape the fusion is for: B = 16, S = 1 024, M = 80 000 negatives shared by every item (Bn = 1), D = 12.
Each against
  * the reference formula (nutil.py:368-385: the (B, 1 + M, S) logits, F.cross_entropy) under torch autograd on the same
    device and the same inputs, the shared negatives expanded as a view;
  * the launch floor: three one-element fills, what three launches cost whatever they compute;
  * the exponential floor: the exponentials the rule asks for (B S M forward, twice that backward) over the rate at which the
    chip's transcendental units could issue them — CUs x 16 lanes a clock at the reported clock.  exp32 itself is not a
    transcendental instruction but a dozen fused multiply-adds, so this floor is below what the kernels can reach.
Peak memory (torch.cuda.max_memory_allocated beyond what was allocated before the call) of both routes goes into the same
record.  A round is `calls` forward+backward calls between two events, after one warm-up call of every route; the record holds
the median, the fastest and the slowest round per call.  The fused gradients are compared with torch's before timing.  No
threshold: the record is the measurement."""
import argparse, json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from imagesequenceregistrationfor6dposeestimationlabeling_amd import losses, ops
from tests import contrastive_ref as cr


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


def peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def case(name, B, S, M, D, Bn, dev, rounds, calls):
    rng = np.random.default_rng(1)
    q, k, n = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in cr.inputs(rng, B, S, M, D, Bn))

    def fused():
        q.grad = k.grad = n.grad = None
        losses.contrastive_loss(q, k, n).backward()

    def reference():
        q.grad = k.grad = n.grad = None
        cr.torch_loss(q, k, n, 1e-3).backward()

    fused()
    ours = [x.grad.clone() for x in (q, k, n)]
    reference()
    rel = [float((a - x.grad).abs().max() / x.grad.abs().max()) for a, x in zip(ours, (q, k, n))]
    one = torch.empty(1, dtype=torch.int32, device=dev)
    props = torch.cuda.get_device_properties(dev)
    clock_hz = (getattr(props, "clock_rate", 0) or 2400000) * 1e3
    exps = 3.0 * B * S * M
    rec = {"case": name, "B": B, "S": S, "M": M, "D": D, "Bn": Bn, "column_splits": ops.contrastive_column_splits(B, S, M, D, Bn),
           "largest_gradient_difference_from_torch_relative_to_the_largest_gradient": {"dq": rel[0], "dk": rel[1], "dn": rel[2]}}
    rec["fused_events"] = timed(fused, rounds, calls)
    rec["torch_events"] = timed(reference, rounds, max(calls // 3, 2))
    rec["launch_floor_three_fills_events"] = timed(lambda: (one.fill_(1), one.fill_(1), one.fill_(1)), rounds, calls)
    rec["fused_events_again"] = timed(fused, rounds, calls)
    rec["exponentials"] = exps
    rec["exponential_floor_ms"] = round(exps / (props.multi_processor_count * 16 * clock_hz) * 1e3, 4)
    rec["exponential_floor_assumes"] = f"{props.multi_processor_count} CUs x 16 lanes a clock at {clock_hz / 1e6:.0f} MHz"
    rec["flop_forward_and_backward"] = 2.0 * B * S * M * D * 5                    # two forward passes, two backward, one p n / p q each
    rec["fused_peak_bytes"] = peak(fused, dev)
    rec["torch_peak_bytes"] = peak(reference, dev)
    ms = rec["fused_events"]["median_ms"]
    rec["torch_over_fused"] = round(rec["torch_events"]["median_ms"] / ms, 3)
    rec["fused_over_launch_floor"] = round(ms / rec["launch_floor_three_fills_events"]["median_ms"], 2)
    rec["fused_over_exponential_floor"] = round(ms / rec["exponential_floor_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    rows = [case("trainPose.py: 16 x 1 024 queries, 1 024 negatives per item", 16, 1024, 1024, 12, 16, dev, a.rounds, a.calls),
            case("every negative: 16 x 1 024 queries, 80 000 shared negatives", 16, 1024, 80000, 12, 1, dev, a.rounds, max(a.calls // 5, 2))]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"what": "losses.contrastive_loss(q, k, n).backward() against the reference formula under torch autograd on the same "
                               "device and inputs, the launch floor (three one-element fills) and the exponential floor (3 B S M "
                               "exponentials at CUs x 16 lanes a clock).  HIP events around `calls_per_round` forward+backward calls, "
                               "per call; one process; peak bytes beyond what was allocated before the call",
                       "device": torch.cuda.get_device_name(0),
                       "not_measured": "the three kernels apart (forward, rows, columns); hardware counters (VALU utilisation, LDS "
                                       "bank conflicts, occupancy); D other than 12; B S other than 16 384; the loss inside a training "
                                       "step of trainPose.py (the encoder and the key field are torch modules there)",
                       "cases": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
