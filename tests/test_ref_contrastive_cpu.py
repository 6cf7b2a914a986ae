"""CPU: the host build of the contrastive loss against tests/golden/ref_contrastive.npz — the reference's own
returnCrossEntropyWithNeg, returnCrossEntropy and returnCrossEntropy2 (nutil.py:349-403), executed under torch autograd in
f32 and f64 by tests/golden/make_ref_losses.py.

The project's standing bound: the host build's loss and each gradient array lie within 4 x the reference's own f32-to-f64
deviation, as the maximum over the array and against the f64 run; the scalar loss gets a floor of one f32 ulp of its value,
because an f32 result cannot be held closer.  No element is excused.  The host entries are driven as losses.py drives the
device ones: scale = 1 / 1000 as an f64, applied to the f64 mean before the one rounding of the loss; the gather
k1[:, negKeys] of the two own-key functions is done here, and dn is added back into dk at negKeys (the gather's gradient).
The measured ratios are in profiles/contrastive_parity.json (written when ISR_RECORD_PARITY is set)."""
import numpy as np
import pytest

from imagesequenceregistrationfor6dposeestimationlabeling_amd import ops
from tests import contrastive_ref as cr
from tests.contrastive_ref import ROOT, f32, f64

WITH_NEG = ("a03", "a1", "a3", "b1", "c1", "d32")
OWN_KEYS = ("e05", "e1", "f2")


@pytest.fixture(scope="module")
def golden():
    return np.load(ROOT / "tests" / "golden" / "ref_contrastive.npz")


def host_loss_and_grads(q, k, n):
    m, t, _, _, loss = ops.contrastive_forward_host(q, k, n, 1 / 1000)
    dq, dk, dn = ops.contrastive_backward_host(q, k, n, m, t, None, 1 / 1000)
    return loss, dq, dk, dn


def check(golden, tag, loss, grads):
    ratios = {}
    l64, e = float(golden[f"{tag}_loss_f64"]), float(golden[f"{tag}_loss_eref"])
    dev = abs(float(loss) - l64)
    bound = max(cr.PARITY_MARGIN * e, cr.ulp32(l64))
    ratios["loss_over_its_bound"] = dev / bound
    print(f"{tag}: loss {float(loss):.9g} against f64 {l64:.9g}: deviation {dev:.3e}, reference f32 {e:.3e}, ulp {cr.ulp32(l64):.3e}")
    assert dev <= bound
    for name, got in grads.items():
        want, e = golden[f"{tag}_d{name}_f64"], float(golden[f"{tag}_d{name}_eref"])
        assert got.shape == want.shape and got.dtype == f32
        dev = np.abs(got.astype(f64) - want).max()
        ratios["d" + name] = dev / e
        print(f"{tag}: d{name} deviation {dev:.3e}, reference f32 {e:.3e}, ratio {dev / e:.2f}")
        assert e > 0 and dev <= cr.PARITY_MARGIN * e
    cr.record("host_against_reference_f64", {tag: {k: round(float(v), 3) for k, v in ratios.items()}})


@pytest.mark.parametrize("tag", WITH_NEG)
def test_with_neg_of_the_reference(hip_lib, golden, tag):
    q, k, n = golden[f"{tag}_q"], golden[f"{tag}_k"], golden[f"{tag}_n"]
    loss, dq, dk, dn = host_loss_and_grads(q, k, n)
    check(golden, tag, loss, {"q": dq, "k": dk, "n": dn})


@pytest.mark.parametrize("tag", OWN_KEYS)
def test_own_keys_of_the_reference(hip_lib, golden, tag):
    q, k, keys = golden[f"{tag}_q"], golden[f"{tag}_k"], golden[f"{tag}_negKeys"]
    if tag != "f2":
        import torch
        torch.manual_seed(int(golden["seed"][0]))                          # the recorded draw is torch's under this seed
        drawn = torch.randperm(k.shape[1], dtype=torch.int64)[0: int(k.shape[1] * float(golden[f"{tag}_negFrac"][0]))]
        assert np.array_equal(drawn.numpy(), keys)
    assert len(np.unique(keys)) == len(keys)
    loss, dq, dk, dn = host_loss_and_grads(q, k, np.ascontiguousarray(k[:, keys]))
    dk = dk.copy()
    dk[:, keys] += dn                                                      # the gather's gradient: distinct indices
    check(golden, tag, loss, {"q": dq, "k": dk})
