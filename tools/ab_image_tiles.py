#!/usr/bin/env python3
"""In-process A/B of the image-tile map (drs_debug_conv_image_tiles) per layer of Dilated8Pooling, forward (without tile statistics,
as at inference: a launch that writes them keeps spatial tiles) and input gradient.
Arms: off (spatial tiles, tap rows skipped) and g = 4, 5, 6, 7 (2^g images x 128 >> g columns per tile, tap rows and columns
skipped).  The arms alternate inside every repeat; a repeat's time is the best of 3 timed launches after one untimed; per arm the
median, minimum and maximum over the repeats are kept, and the outputs of every arm are compared bitwise with the off arm's in the
same run.  A layer gains only if its best arm's MAXIMUM is below the off arm's MINIMUM.
    python tools/ab_image_tiles.py [B=128] [S=64] [repeats=7] [out=ab.json]"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drs_amd import _lib
_lib = _lib.dev()
from drs_amd.nets import Plan
DEV = "cuda:0"
ARMS = [("off", 0), ("g4", 4), ("g5", 5), ("g6", 6), ("g7", 7)]


def main(B=128, S=64, repeats=7, out=None):
    L_ = _lib.load()
    plan = Plan("dilated_grsl_rate8", 5, 6)
    st = torch.cuda.current_stream(DEV).cuda_stream
    M = B * S * S
    ws_n = max(_lib.query("drs_conv_workspace_floats", c) for c in (64, 128, 192, 256))
    ws = torch.zeros(ws_n, device=DEV)
    rows = []
    for i, L in enumerate(plan.layers):
        if i == 0:
            continue
        P = L.halo
        x = torch.randn(B * (S + 2 * P) ** 2 * L.cin_k, device=DEV).view(B, S + 2 * P, S + 2 * P, L.cin_k)
        g = torch.randn(B * (S + 2 * P) ** 2 * L.cout, device=DEV).view(B, S + 2 * P, S + 2 * P, L.cout)
        for t in (x, g):          # the zero halo the kernels rely on
            t[:, :P] = 0; t[:, S + P:] = 0; t[:, :, :P] = 0; t[:, :, S + P:] = 0
        w = torch.randn(L.k * L.k * L.cin_k * L.cout, device=DEV) * 0.05
        bias = torch.zeros(L.cout, device=DEV)
        z = torch.zeros(M * max(L.cout, L.cin_k), device=DEV)
        fns = {"fwd": lambda: _lib.call("drs_conv_forward_ws", x.data_ptr(), B, S, P, L.cin_k, 0, w.data_ptr(), bias.data_ptr(), L.k, L.rate, L.pad_b,
                                        L.cin_k, L.cout, z.data_ptr(), L.cout, 0, 0, None, ws.data_ptr(), ws_n, st),
               "dgrad": lambda: _lib.call("drs_conv_forward_ws", g.data_ptr(), B, S, P, L.cout, 0, w.data_ptr(), None, L.k, L.rate, L.pad_a, L.cout,
                                          L.cin_k, z.data_ptr(), L.cin_k, 0, 0, None, ws.data_ptr(), ws_n, st)}
        for dname, f in fns.items():
            n_out = M * (L.cout if dname == "fwd" else L.cin_k)
            times = {a: [] for a, _ in ARMS}
            ref, same = None, {}
            for r in range(repeats):
                for a, gsel in ARMS:
                    L_.drs_debug_conv_image_tiles(gsel)
                    best = 1e9
                    for rep in range(4):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(); f(); e1.record()
                        torch.cuda.synchronize()
                        if rep:
                            best = min(best, e0.elapsed_time(e1))
                    times[a].append(best)
                    if r == 0:
                        if a == "off":
                            ref = z[:n_out].clone()
                        same[a] = bool(torch.equal(z[:n_out], ref))
            row = {"layer": L.name, "dir": dname, "k": L.k, "rate": L.rate, "cin": L.cin_k if dname == "fwd" else L.cout,
                   "cout": L.cout if dname == "fwd" else L.cin_k, "bitwise_equal_to_off": same,
                   "ms": {a: {"median": float(np.median(t)), "min": min(t), "max": max(t)} for a, t in times.items()}}
            rows.append(row)
            print("%-6s %-5s " % (L.name, dname) + " | ".join("%s %.3f [%.3f, %.3f]%s" % (a, row["ms"][a]["median"], row["ms"][a]["min"], row["ms"][a]["max"],
                                                                                     "" if same[a] else " BITS DIFFER") for a, _ in ARMS), flush=True)
        del x, g
    L_.drs_debug_conv_image_tiles(-1)
    tot = {a: sum(r["ms"][a]["median"] for r in rows) for a, _ in ARMS}
    print("total (medians) " + " | ".join("%s %.3f" % (a, tot[a]) for a, _ in ARMS) + " ms")
    if out:
        json.dump({"B": B, "S": S, "repeats": repeats, "rows": rows, "total_median_ms": tot}, open(out, "w"), indent=1)


if __name__ == "__main__":
    kw = dict(a.split("=") for a in sys.argv[1:])
    main(int(kw.get("B", 128)), int(kw.get("S", 64)), int(kw.get("repeats", 7)), kw.get("out"))
