#!/usr/bin/env python3
"""Randomised shapes through the average-pool and squeeze-and-excitation entry points (forward and backward), against the fp64
oracle: the checks are those of tests/test_gpu_pointwise_oplevel.py (called as functions), the shapes are drawn here -- channels
4..576 in steps of 4, reduced widths 1..C/2, odd windows 1..9, sides 1..33, batches 1..5, halos 0..8, output slices at any
multiple of 4 channels inside a wider slab.  Test infrastructure.
    python tests/fuzz/fuzz_se_avgpool.py [n=200] [seed=0]"""
import os, sys, traceback
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from drs_amd import _lib
import test_gpu_pointwise_oplevel as G


def main(n=200, seed=0):
    rng = np.random.default_rng(seed)
    nbad = 0
    for i in range(n):
        C = 4 * int(rng.integers(1, 145))
        S = int(rng.integers(1, 34))
        B = int(rng.integers(1, 6))
        P = int(rng.integers(0, 9))
        while B * S * S * C > 2.5e6:
            S = max(1, S - 3)
        coff = 4 * int(rng.integers(0, 9))
        ld = coff + C + 4 * int(rng.integers(0, 9))
        if i % 2 == 0:
            args = (C, 2 * int(rng.integers(0, 5)) + 1, B, S, P, ld, coff)
            name, fn = "avg_pool", G.test_avg_pool_forward_backward
        else:
            args = (C, int(rng.integers(1, max(1, C // 2) + 1)), B, S, P, ld, coff)
            name, fn = "se", G.test_se_forward_backward
        try:
            fn(_lib, *args)
        except AssertionError:
            nbad += 1
            tb = traceback.format_exc().strip().splitlines()
            print("\nFAIL", name, args, "|", tb[-3].strip()[:150], "|", tb[-1][:200], flush=True)
    print("\n%d cases, %d failed" % (n, nbad))
    sys.exit(1 if nbad else 0)


if __name__ == "__main__":
    kw = dict(a.split("=") for a in sys.argv[1:])
    main(int(kw.get("n", 200)), int(kw.get("seed", 0)))
