#!/usr/bin/env python3
"""Writes tests/golden/field_host_bits.npz: the bits of the host entries of the key field and the density field as the
library gives them NOW, with the small inputs beside them.  tests/test_field_bits_cpu.py holds the inputs' construction and
the list of what is pinned; this script only runs it and saves.  The file pins a state of the arithmetic: regenerate it only
with a change that is meant to change a bit, and say so.
Run from the repo root:  python tests/golden/make_field_host_bits.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from imagesequenceregistrationfor6dposeestimationlabeling_amd import _capi  # noqa: E402
from tests import test_field_bits_cpu as t  # noqa: E402


def main():
    inp = t.small_inputs()
    out = t.compute(_capi.lib(), inp)
    for name in t.DENSITY_FIELDS:
        for thr in t.THRESHOLDS:
            print(f"{name} threshold {thr:g}: {int(out[f'{name}_march_{thr:g}_hit'].sum())} of 5 rays hit; share of densities "
                  f"above 0.2: {float((out[f'{name}_march_{thr:g}_densities'] > 0.2).mean()):.2f}")
    np.savez_compressed(t.GOLDEN, **inp, **out)
    print(t.GOLDEN, t.GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
