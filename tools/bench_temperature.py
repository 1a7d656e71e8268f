#!/usr/bin/env python3
"""Per-launch time of the two kernels of temperature scaling on an h x w x K accumulator (default 6000 x 6000 x 6: a
Potsdam tile), in one process: drs_temperature_stats (one evaluation of the fit on one map: both launches), and
drs_stitch_finalize_scores_t with all four outputs at beta = 0.5 against the same call at beta = 1, which runs the unchanged
score_maps_kernel and is the yardstick.  The accumulator holds sums of logits (prob=0) or of probabilities (prob=1), occur in 1..4, labels
in 0..K with K the ignored byte.  Alternating order, `rounds` rounds of `n` back-to-back launches per variant after a warm-up, HIP events
on the launch stream.  Prints one JSON line and writes it to out= (default profiles/temperature/cost.json) with the clocks the device
reports.  The statistics read 4K + 5 bytes per pixel, the finalising pass reads 4K + 4 and writes 4; the line carries the GB/s that
makes.

    python tools/bench_temperature.py [h=6000] [w=6000] [K=6] [prob=0] [n=20] [rounds=5] [out=profiles/temperature/cost.json]"""
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
    truth = torch.randint(0, K + 1, (npix,), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    maps = [torch.zeros(npix, dtype=torch.uint8, device=DEV) for _ in range(4)]
    scratch = torch.zeros(_lib.query("drs_temperature_scratch_doubles", npix), dtype=torch.float64, device=DEV)
    out = torch.zeros(5, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream

    def run(which):
        if which == "temperature_stats":
            _lib.call("drs_temperature_stats", sums.data_ptr(), occur.data_ptr(), truth.data_ptr(), npix, K, prob, K, 0.5, scratch.data_ptr(),
                      out.data_ptr(), st)
        else:
            _lib.call("drs_stitch_finalize_scores_t", sums.data_ptr(), occur.data_ptr(), h, w, K, prob, 0.5 if which == "scores_t_beta_half" else 1.0,
                      *[m.data_ptr() for m in maps], st)
    ms = {k: [] for k in ("scores_t_beta_one", "scores_t_beta_half", "temperature_stats")}
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
    nbytes = {"scores_t_beta_one": npix * (4 * K + 4 + 4), "scores_t_beta_half": npix * (4 * K + 4 + 4), "temperature_stats": npix * (4 * K + 4 + 1)}
    res = {"shape": [h, w, K], "sums_are_prob": prob, "launches_per_round": n, "ms_per_launch": ms, "median_ms": med,
           "gb_per_s": {k: round(nbytes[k] / med[k] / 1e6, 1) for k in med},
           "ratio_beta_half_over_beta_one": round(med["scores_t_beta_half"] / med["scores_t_beta_one"], 4),
           "ratio_stats_over_beta_one": round(med["temperature_stats"] / med["scores_t_beta_one"], 4),
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
        sys.exit("bench_temperature.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("h", 6000)), int(kw.get("w", 6000)), int(kw.get("K", 6)), int(kw.get("prob", 0)), int(kw.get("n", 20)),
         int(kw.get("rounds", 5)), kw.get("out", os.path.join(ROOT, "profiles", "temperature", "cost.json")))
