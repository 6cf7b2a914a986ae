"""The key field of refine_pose (fields.KeyField, isr_field_eval) against the same weights as a torch module:
    python tools/bench_key_field.py [--out profiles/key_field_vs_torch.json] [--reps 10]
Widths 3 -> 256 -> 256 -> 256 -> 12 (the reference's feature head: Siren(3, 12, hidden 256, 2 hidden layers), nerf.py:201-202;
sine layers of omega 30, a linear last layer), B = 32 images x 20 000 visible points.
  * one KeyField.batched_customForward call over the block's 640 000 points (HIP events, median and spread over `reps`), and
    its FLOP/s over the f32 matrix peak;
  * the torch module driven as refine_poses drives any other field: once per image, 16 chunk forwards each (nerf.py:404-457)
    — HIP events, and the host's wall time around the same loop (512 forwards of a few launches each);
  * the field's share of a sequence.estimate_and_refine block (B = 32, optimizer="device", the renderer's render_batch): the
    block's wall time with the KeyField and with the torch module, and the field_eval time from ops' event timers.
No threshold: the record is the measurement."""
import argparse, json, os, statistics, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops, sequence, synth
from imagesequenceregistrationfor6dposeestimationlabeling_amd.fields import KeyField
from bench_render import event_timed, stats, surf_block
from tests.field_ref import TorchField, siren_params

WIDTHS = (3, 256, 256, 256, 12)
OMEGAS = (30.0, 30.0, 30.0, None)
PEAK_F32_MATRIX = 157.3e12          # MI355X, v_mfma_f32_32x32x2_f32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--block-reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no HIP device: nothing is measured"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    Ws, bs = siren_params(WIDTHS, OMEGAS, seed=11)
    field = KeyField(Ws, bs, OMEGAS, dev)
    module = TorchField(Ws, bs, OMEGAS).to(dev)
    B, per = 32, 20_000
    x = torch.from_numpy(rng.uniform(-0.9, 0.9, (B * per, 3)).astype(np.float32)).to(dev)
    one = lambda: field.batched_customForward(x)
    loop = lambda: [module.batched_customForward(x[b * per:(b + 1) * per].clone()).detach().clone() for b in range(B)]
    got = one()
    ref = torch.cat(loop())
    torch.cuda.synchronize()
    diff = float((got - ref).abs().max())
    kf = stats(event_timed(one, a.reps))
    tl = stats(event_timed(loop, a.reps))
    wall = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    flops = B * per * ops.field_flops(WIDTHS)
    row = {"widths": list(WIDTHS), "omegas": list(OMEGAS), "B": B, "points_per_image": per, "flop": flops,
           "key_field_one_call_events": kf, "torch_per_image_16_chunks_events": tl, "torch_per_image_16_chunks_wall": stats(wall),
           "key_field_tflops": round(flops / (kf["median_ms"] * 1e-3) / 1e12, 2),
           "key_field_share_of_f32_matrix_peak": round(flops / (kf["median_ms"] * 1e-3) / PEAK_F32_MATRIX, 4),
           "torch_tflops": round(flops / (tl["median_ms"] * 1e-3) / 1e12, 2),
           "torch_over_key_field_events": round(tl["median_ms"] / kf["median_ms"], 3),
           "max_abs_difference_between_the_two": diff}
    print(json.dumps(row), flush=True)

    # the field's share of a useSurfEval block: the same weights behind both objects
    e = WIDTHS[-1]
    s = surf_block(B, e, rng, dev)
    pts_d, keys_d = torch.from_numpy(s["v"].astype(np.float32)).to(dev), torch.from_numpy(s["keys"]).to(dev)
    kv = field(torch.from_numpy((s["v"] * 1.8 / s["obj"].diameter).astype(np.float32)).to(dev))
    share = {"B": B, "res": 224, "faces": int(len(s["obj"].mesh.faces))}
    for name, nerf in (("key_field", field), ("torch_module", module)):
        args = (s["ml"], s["q"], pts_d, s["nrm"], keys_d, synth.diameter(s["v"]), s["K"], s["rend"], 0, s["obj"], nerf, kv,
                s["v"][::10], s["Rg"], s["tg"])
        kw = dict(estimate_kw=dict(max_pose_evaluations=1000), refine_kw=dict(optimizer="device"))
        sequence.estimate_and_refine(*args, **kw)
        block_ms, field_ms, calls, refined = [], [], 0, 0
        for _ in range(a.block_reps):
            ops.enable_timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = sequence.estimate_and_refine(*args, **kw)
            torch.cuda.synchronize()
            block_ms.append((time.perf_counter() - t0) * 1e3)
            rec = ops.drain_timing()
            ops.enable_timing(False)
            if "field_eval" in rec:
                calls = rec["field_eval"][0]
                field_ms.append(rec["field_eval"][1])
            refined = int(out["refined"].sum())
        share[name] = {"block_wall": stats(block_ms), "refined": refined}
        if field_ms:
            share[name].update(field_eval_calls=calls, field_eval_events=stats(field_ms),
                               field_share_of_block=round(statistics.median(field_ms) / statistics.median(block_ms), 5))
    print(json.dumps(share), flush=True)
    doc = {"what": "fields.KeyField (one isr_field_eval launch per block) against the same weights as a torch module called per "
                   "image in 16 chunks, and the field's share of an estimate_and_refine block",
           "device": torch.cuda.get_device_name(0), "f32_matrix_peak_flops": PEAK_F32_MATRIX, "field": row,
           "estimate_and_refine_share": share}
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
