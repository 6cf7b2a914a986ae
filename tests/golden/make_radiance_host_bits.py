#!/usr/bin/env python3
"""Writes tests/golden/radiance_host_bits.npz: the words of the host entries of the radiance field, of the emission-absorption
march and its backward and of the march of given densities as the library gives them NOW.  tests/test_radiance_bits_cpu.py
holds the inputs' construction (all of them remade from integer arithmetic, none stored) and the list of what is pinned; this
script only runs it and saves.  The file pins a state of the arithmetic: regenerate it only with a change that is meant to
change a bit, and say so.
Run from the repo root:  python tests/golden/make_radiance_host_bits.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import test_radiance_bits_cpu as t  # noqa: E402


def main():
    out = t.compute()
    for name in t.RADIANCE_FIELDS:
        for thr, n in t.hits(out, name).items():
            print(f"{name} threshold {thr:g}: {n} of 5 rays hit")
    for P in t.MARCH_P:
        for thr in t.THRESHOLDS:
            print(f"given densities P {P} threshold {thr:g}: {int(out[f'given_P{P}_{thr:g}_front_hit'].sum())} of {t.MARCH_N} rays hit")
    np.savez_compressed(t.GOLDEN, **out)
    print(t.GOLDEN, t.GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
