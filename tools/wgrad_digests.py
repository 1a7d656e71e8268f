#!/usr/bin/env python3
"""SHA-256 digests of what drs_conv_wgrad writes -- the filter gradient and the split slab -- for seeded inputs: the yardstick of a
change to the filter-gradient kernels that must leave every bit where it was (run it on the tree before and on the tree after, on
the same machine, one process each, and compare the two JSON objects entry for entry).  Only drs_conv_wgrad, drs_conv_wgrad_splits
and the development switches drs_debug_wgrad_variant / drs_debug_wgrad_seg are called, so the same file runs on either tree.

Cases:
  rows/*     one (k, cin, cout) per tile shape drs_conv_wgrad dispatches (the rows of
             tests/test_gpu_ops.py::test_filter_gradient_chunk_walk_over_patch_sides), rate 2, each at the four sides 9 x 3 images
             (division path, ragged last chunk), 21 x 2 (incremental tables below 32), 32 x 2 (affine), 45 x 1 (segments / tables)
  layers/*   the eight layers of Dilated8Pooling at 16 x 64 x 64 and at 16 x 45 x 45
Each through the product library (its own pick of the form) and through the development library with the form forced:
variant 0 (register-staged), variant 1 with the row segments (seg 1) and with the offset tables (seg 0).
    python tools/wgrad_digests.py [out=FILE]
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drs_amd import _lib  # noqa: E402
from drs_amd.nets import Plan  # noqa: E402

DEV = "cuda:0"
SHAPES = [(3, 64, 128), (3, 64, 192), (3, 64, 64), (3, 64, 96), (1, 64, 128), (1, 64, 64), (2, 16, 96), (1, 96, 128), (1, 32, 64), (1, 96, 96)]
SIDES = [(9, 3), (21, 2), (32, 2), (45, 1)]
FORMS = [("v0", 0, 1), ("v1seg", 1, 1), ("v1tab", 1, 0)]


def sha(t):
    x = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(str((x.dtype.str, x.shape)).encode() + x.tobytes()).hexdigest()


def slab_with_halo(rng, B, S, P, C):
    x = np.zeros((B, S + 2 * P, S + 2 * P, C), dtype=np.float32)
    x[:, P:P + S, P:P + S, :] = rng.normal(size=(B, S, S, C)).astype(np.float32)
    return torch.from_numpy(x.reshape(-1)).to(DEV)


def case(out, name, B, S, k, rate, pb, P, cin, cout):
    rng = np.random.default_rng([B, S, k, rate, cin, cout])
    xd, gd = slab_with_halo(rng, B, S, P, cin), slab_with_halo(rng, B, S, P, cout)
    st = torch.cuda.current_stream(DEV).cuda_stream
    dev = _lib.dev()

    def run(lib, tag):
        nsp = lib.query("drs_conv_wgrad_splits", B, S, k, cin, cout)
        slab = torch.zeros(nsp * k * k * cin * cout, dtype=torch.float32, device=DEV)
        gw = torch.full((k * k * cin * cout,), 7.0, dtype=torch.float32, device=DEV)
        lib.call("drs_conv_wgrad", xd.data_ptr(), B, S, P, cin, 0, gd.data_ptr(), P, cout, 0, k, rate, pb, cin, cin, cout, slab.data_ptr(),
                 gw.data_ptr(), st)
        torch.cuda.synchronize()
        out["%s/%s/grad" % (name, tag)] = sha(gw)
        out["%s/%s/slab" % (name, tag)] = sha(slab)

    run(_lib, "product")
    try:
        for tag, variant, seg in FORMS:
            dev.drs_debug_wgrad_variant(variant)
            dev.drs_debug_wgrad_seg(seg)
            run(dev, tag)
    finally:
        dev.drs_debug_wgrad_variant(-1)
        dev.drs_debug_wgrad_seg(1)


def main(path):
    _lib.load()
    out = {}
    for k, cin, cout in SHAPES:
        pb = (k - 1) * 2 // 2          # `same` padding of the dilated window, rate 2: (k - 1) * rate pixels, the smaller half in front
        P = (k - 1) * 2 - pb
        for S, B in SIDES:
            case(out, "rows/k%d-%d-%d/%dx%d" % (k, cin, cout, S, B), B, S, k, 2, pb, max(pb, P), cin, cout)
    plan = Plan("dilated_grsl_rate8", 5, 6, first_cin_pad=8)
    for S in (64, 45):
        for L in plan.layers:
            case(out, "layers/%s/16x%d" % (L.name, S), 16, S, L.k, L.rate, L.pad_b, L.halo, L.cin_k, L.cout)
    text = json.dumps(out, indent=0, sort_keys=True)
    if path:
        with open(path, "w") as f:
            f.write(text + "\n")
    print("%d digests, sha256 of all: %s" % (len(out), hashlib.sha256(text.encode()).hexdigest()))


if __name__ == "__main__":
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(kw.get("out"))
