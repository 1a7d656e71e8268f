#!/usr/bin/env python3
"""What the boundary table (drs_boundary_histogram) costs, in one process on one device: a synthetic pair of blob maps
(`mosaic` x `mosaic`, K = 6: a Voronoi truth with a thin ignore band along its boundaries, the prediction the same cells with
displaced seeds and some speckle -- the shape of a real validation pair: most pixels far from every contour), and HIP-event times of
  - drs_boundary_histogram at the default distances (1, 2, 4, 8) and at full reach (1, 2, 4, 8, 16),
  - drs_boundary_distance of one map at reach 8,
  - drs_confusion on the same buffers (the count the table's total repeats) and
  - a device-to-device copy of the two maps (what reading them once and writing them once costs),
each launched `warmup` times untimed, then `reps` times, one event pair per launch; the median and the extremes are reported, the
arms interleaved so that a drift of the clocks meets all of them.  The tables are checked against each other (the sum over the bins
is drs_confusion's matrix) and a digest of each is kept.  Prints one JSON line and writes it to out=.

    python tools/bench_boundary.py [mosaic=6000] [reps=15] [warmup=3] [out=profiles/boundary_scores/bench.json]"""
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drs_amd import _lib, loops, metrics as MT, patches as P  # noqa: E402

DEV = "cuda:0"
K, IGNORE = 6, 6
OPTIONS = ("mosaic", "reps", "warmup", "out")
INFERENCE_S = 4.14       # whole-map overlap-tile inference of such a mosaic (profiles/r06), the yardstick of DESIGN.md 8a.7


def blob_maps(n, seed=0, cells=400):
    """(truth, pred) uint8 [n][n] on the device: Voronoi cells of `cells` seeds (about n / 20 pixels across), made on the device in row
    bands; the truth's 4-neighbour boundary pixels carry IGNORE; the prediction's seeds are displaced by up to 6 pixels and one pixel
    in 4000 is speckle"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pts = torch.randint(0, n, (cells, 2), generator=g).float()
    moved = pts + torch.randint(-6, 7, (cells, 2), generator=g).float()
    labels = (torch.randperm(cells, generator=g) % K).to(torch.uint8).to(DEV)
    xs = torch.arange(n, device=DEV, dtype=torch.float32)

    def voronoi(p):
        p = p.to(DEV)
        out = torch.empty((n, n), dtype=torch.uint8, device=DEV)
        for y0 in range(0, n, 64):
            ys = torch.arange(y0, min(n, y0 + 64), device=DEV, dtype=torch.float32)
            d = (ys[:, None, None] - p[None, None, :, 0]) ** 2 + (xs[None, :, None] - p[None, None, :, 1]) ** 2
            out[y0:y0 + len(ys)] = labels[d.argmin(dim=-1)]
        return out
    truth, pred = voronoi(pts), voronoi(moved)
    edge = torch.zeros((n, n), dtype=torch.bool, device=DEV)
    edge[1:] |= truth[1:] != truth[:-1]
    edge[:-1] |= truth[:-1] != truth[1:]
    edge[:, 1:] |= truth[:, 1:] != truth[:, :-1]
    edge[:, :-1] |= truth[:, :-1] != truth[:, 1:]
    truth[edge] = IGNORE
    speck = torch.rand((n, n), generator=g) < 1.0 / 4000
    speck = speck.to(DEV)
    pred[speck] = (pred[speck] + 1) % K
    return truth.contiguous(), pred.contiguous()


def main(n, reps, warmup, out_path):
    assert torch.cuda.is_available(), "bench_boundary.py measures on the device: there is no CPU path"
    _lib.load()
    truth, pred = blob_maps(n)
    st = torch.cuda.current_stream(DEV).cuda_stream
    near, far = P.BOUNDARY_DEFAULT, P.BOUNDARY_DEFAULT + (16,)
    tables = {d: torch.zeros((len(d) + 1, len(d) + 1, K, K), dtype=torch.int64, device=DEV) for d in (near, far)}
    d2 = torch.empty(n * n, dtype=torch.int16, device=DEV)
    conf = torch.zeros(K * K, dtype=torch.int32, device=DEV)
    copy = torch.empty((2, n, n), dtype=torch.uint8, device=DEV)
    both = torch.stack([truth, pred])
    arms = {
        "histogram_d8": lambda: loops.boundary_histogram(truth, pred, n, n, K, IGNORE, near, hist=tables[near], stream=st),
        "histogram_d16": lambda: loops.boundary_histogram(truth, pred, n, n, K, IGNORE, far, hist=tables[far], stream=st),
        "distance_r8": lambda: _lib.call("drs_boundary_distance", truth.data_ptr(), n, n, 8, d2.data_ptr(), st),
        "confusion": lambda: _lib.call("drs_confusion", truth.data_ptr(), pred.data_ptr(), None, n * n, K, IGNORE, conf.data_ptr(), st),
        "copy_two_maps": lambda: copy.copy_(both),
    }
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    launches = warmup + reps
    cm = conf.cpu().numpy().reshape(K, K).astype(np.int64)
    assert cm.sum() % launches == 0
    cm //= launches
    res = {"workload": "%dx%d synthetic blob map pair, K = %d, ignore band along the truth's boundaries" % (n, n, K),
           "reps": reps, "warmup": warmup, "inference_s_of_such_a_map": INFERENCE_S}
    for name, t in times.items():
        res[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    for d, key in ((near, "histogram_d8"), (far, "histogram_d16")):
        h = tables[d].cpu().numpy()
        assert (h % launches == 0).all()
        h //= launches
        assert (h.sum(axis=(0, 1)) == cm).all(), "the table's total is not drs_confusion's matrix"
        s = MT.boundary_scores(h, d)
        res[key + "_share_of_inference"] = round(res[key + "_ms"]["median"] / 1e3 / INFERENCE_S, 6)
        res[key + "_band_pixels"] = [b["count"] for b in s["bands"]]
        res[key + "_boundary_iou"] = [round(b["boundary_iou"], 6) for b in s["bands"]]
        res[key + "_digest"] = int((h.reshape(-1) * (np.arange(h.size, dtype=np.int64) % 1009 + 1)).sum() % (1 << 61))
    res["counted_pixels"] = int(cm.sum())
    res["mean_iou"] = round(MT.mean_iou(cm), 6)
    res["histogram_d8_over_confusion"] = round(res["histogram_d8_ms"]["median"] / res["confusion_ms"]["median"], 3)
    res["histogram_d8_over_copy"] = round(res["histogram_d8_ms"]["median"] / res["copy_two_maps_ms"]["median"], 3)
    res["device"] = torch.cuda.get_device_name(DEV)
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    bad = [a for a in sys.argv[1:] if "=" not in a or a.split("=", 1)[0] not in OPTIONS]
    if bad:
        sys.exit("bench_boundary.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("mosaic", 6000)), int(kw.get("reps", 15)), int(kw.get("warmup", 3)),
         kw.get("out", os.path.join(ROOT, "profiles", "boundary_scores", "bench.json")))
