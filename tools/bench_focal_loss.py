#!/usr/bin/env python3
"""Per-launch time of the fused classifier at the headline step's shape (128 x 64 x 64, C = 256, K = 6: the LDS-DMA form, training) in
the three loss modes -- plain, class-weighted, focal -- and, with parent=<path to another build's libdrs_hip.so>, of
that build's drs_classifier_loss_focal in the same three modes beside them (parent_plain, parent_weighted, parent_focal against
new_*).  Alternating order, `rounds` rounds of `n` back-to-back launches per variant after a warm-up, HIP events on the launch
stream; prints one JSON line.  The two builds' kernels carry the same names (classifier_dma_kernel<4, true, 0 / 1 / 2>), so a kernel
trace of this run cannot tell them apart: the event times are the comparison.

    python tools/bench_focal_loss.py [parent=/path/to/libdrs_hip.so] [B=128] [S=64] [C=256] [K=6] [gamma=2] [n=50] [rounds=5]"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drs_amd import _lib  # noqa: E402
DEV = "cuda:0"
OPTIONS = ("parent", "B", "S", "C", "K", "gamma", "n", "rounds")


def load_parent(path):
    """a second build of the library in this process: it exports the same symbol names, which is safe because ctypes opens a
    library RTLD_LOCAL -- each handle resolves its own drs_classifier_loss_focal"""
    lib = ctypes.CDLL(path)
    lib.drs_classifier_loss_focal.restype, lib.drs_classifier_loss_focal.argtypes = _lib.SIGNATURES["drs_classifier_loss_focal"]
    return lib


def main(parent, B, S, C, K, gamma, n, rounds):
    new = _lib.load()
    par = load_parent(parent) if parent else None
    M = B * S * S
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    feat = torch.randn(M * C, device=DEV, generator=g)
    w = torch.randn(C * K, device=DEV, generator=g) / 16
    b = torch.zeros(K, device=DEV)
    lab = torch.randint(0, K, (M,), device=DEV, generator=g).to(torch.uint8)
    am = torch.ones(M, dtype=torch.uint8, device=DEV)
    rows = _lib.query("drs_classifier_rows", B, S)
    pred = torch.zeros(M, dtype=torch.uint8, device=DEV)
    gfeat = torch.zeros(M * C, device=DEV)
    dw = torch.zeros(rows * C * K, device=DEV)
    db = torch.zeros(rows * K, device=DEV)
    lp = torch.zeros(rows, dtype=torch.float64, device=DEV)
    conf = torch.zeros(K * K, dtype=torch.int32, device=DEV)
    wc = np.asarray(([0.5, 2.0, 0.0, 1.25, 7.0, 1.0, 3.0, 0.25])[:K], dtype=np.float32)
    st = torch.cuda.current_stream(DEV).cuda_stream
    head = (feat.data_ptr(), B, S, 0, C, 0, C, K, w.data_ptr(), b.data_ptr(), lab.data_ptr(), None, am.data_ptr(), 1.0 / M)
    tail = (None, pred.data_ptr(), gfeat.data_ptr(), C, 0, dw.data_ptr(), db.data_ptr(), lp.data_ptr(), conf.data_ptr(), st)
    mid = {"plain": (None, 0.0), "weighted": (wc.ctypes.data, 0.0), "focal": (None, gamma)}
    libs = ({"parent": par} if par is not None else {}) | {"new": new}

    def run(which):
        build, mode = which.split("_")
        rc = libs[build].drs_classifier_loss_focal(*(head + mid[mode] + tail))
        assert rc == 0, (which, rc)
    out = {"%s_%s" % (build, mode): [] for build in libs for mode in mid}
    for k in out:
        for _ in range(10):
            run(k)
    torch.cuda.synchronize()
    for r in range(rounds):
        for k in (list(out) if r % 2 == 0 else list(out)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            out[k].append(round(e0.elapsed_time(e1) / n, 5))
    print(json.dumps({"shape": [B, S, S, C, K], "gamma": gamma, "launches_per_round": n, "ms_per_launch": out,
                      "median_ms": {k: float(np.median(v)) for k, v in out.items()}}))


if __name__ == "__main__":
    bad = [a for a in sys.argv[1:] if "=" not in a or a.split("=", 1)[0] not in OPTIONS]
    if bad:
        sys.exit("bench_focal_loss.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(kw.get("parent"), int(kw.get("B", 128)), int(kw.get("S", 64)), int(kw.get("C", 256)), int(kw.get("K", 6)), float(kw.get("gamma", 2.0)),
         int(kw.get("n", 50)), int(kw.get("rounds", 5)))
