#!/usr/bin/env python3
"""Per-launch time of the finalize pass of whole-tile inference on an h x w x K accumulator (default 6000 x 6000 x 6: a Potsdam tile):
drs_stitch_finalize (labels only; unchanged by the score maps, so it is the yardstick), drs_stitch_finalize_scores with all four outputs,
and drs_stitch_finalize_scores with labels only.  The accumulator holds sums of logits, occur in 1..4.  Alternating
order, `rounds` rounds of `n` back-to-back launches per variant after a warm-up, HIP events on the launch stream.  Prints one JSON line
and writes it to out= (default profiles/score_maps/cost.json) with the clocks the device reports.  The pass reads 4K + 4 bytes and
writes 1 to 4 per pixel; the line carries the GB/s that makes.

    python tools/bench_score_maps.py [h=6000] [w=6000] [K=6] [prob=0] [n=20] [rounds=5] [out=profiles/score_maps/cost.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drs_amd import _lib  # noqa: E402
DEV = "cuda:0"
OPTIONS = ("h", "w", "K", "prob", "n", "rounds", "out")


def clocks():
    """what the device says about its clocks: the rated one, and the current one where the runtime can read it"""
    rated = getattr(torch.cuda.get_device_properties(DEV), "clock_rate", None)      # kHz, where this torch reports it
    c = {"rated_mhz": None if rated is None else rated / 1000.0}
    try:
        c["current_mhz"] = float(torch.cuda.clock_rate(DEV))
    except Exception as e:      # the management library is optional: say so instead of a number
        c["current_mhz"] = None
        c["current_mhz_unavailable"] = type(e).__name__
    return c


def main(h, w, K, prob, n, rounds, out_path):
    _lib.load()
    npix = h * w
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    occur = torch.randint(1, 5, (npix,), device=DEV, generator=g, dtype=torch.int32)
    sums = torch.randn(npix, K, device=DEV, generator=g) * 2.5
    if prob:
        sums = torch.softmax(sums, dim=1)
    sums = (sums * occur[:, None].float()).reshape(-1).contiguous()
    maps = [torch.zeros(npix, dtype=torch.uint8, device=DEV) for _ in range(4)]
    st = torch.cuda.current_stream(DEV).cuda_stream

    def run(which):
        if which == "finalize":
            _lib.call("drs_stitch_finalize", sums.data_ptr(), occur.data_ptr(), h, w, K, maps[0].data_ptr(), st)
        elif which == "scores_all_four":
            _lib.call("drs_stitch_finalize_scores", sums.data_ptr(), occur.data_ptr(), h, w, K, prob, *[m.data_ptr() for m in maps], st)
        else:
            _lib.call("drs_stitch_finalize_scores", sums.data_ptr(), occur.data_ptr(), h, w, K, prob, maps[0].data_ptr(), None, None, None, st)
    ms = {k: [] for k in ("finalize", "scores_all_four", "scores_labels_only")}
    before = clocks()
    for k in ms:
        for _ in range(3):
            run(k)
    torch.cuda.synchronize()
    for r in range(rounds):
        for k in (list(ms) if r % 2 == 0 else list(ms)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(round(e0.elapsed_time(e1) / n, 5))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    nbytes = {"finalize": npix * (4 * K + 4 + 1), "scores_all_four": npix * (4 * K + 4 + 4), "scores_labels_only": npix * (4 * K + 4 + 1)}
    res = {"shape": [h, w, K], "sums_are_prob": prob, "launches_per_round": n, "ms_per_launch": ms, "median_ms": med,
           "gb_per_s": {k: round(nbytes[k] / med[k] / 1e6, 1) for k in med},
           "ratio_all_four_over_finalize": round(med["scores_all_four"] / med["finalize"], 4),
           "ratio_labels_only_over_finalize": round(med["scores_labels_only"] / med["finalize"], 4),
           "device": torch.cuda.get_device_name(DEV), "clocks_before": before, "clocks_after": clocks()}
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    bad = [a for a in sys.argv[1:] if "=" not in a or a.split("=", 1)[0] not in OPTIONS]
    if bad:
        sys.exit("bench_score_maps.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("h", 6000)), int(kw.get("w", 6000)), int(kw.get("K", 6)), int(kw.get("prob", 0)), int(kw.get("n", 20)),
         int(kw.get("rounds", 5)), kw.get("out", os.path.join(ROOT, "profiles", "score_maps", "cost.json")))
