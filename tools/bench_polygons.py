#!/usr/bin/env python3
"""What the polygon output (drs_polygon_count, drs_polygon_rings, drs_polygon_write behind drs_components) costs, in
one process on one device: a `mosaic` x `mosaic` speckled label map of K = 6 (tools/bench_sieve.py's: Voronoi cells with `speckle` of
the pixels re-drawn), sieved to `min_size` pixels at connectivity 4 (loops.sieve_labels) -- the map a user would trace -- and, for the
worst case of the doubling's traffic, the unsieved map too.  HIP-event times per map of
  - drs_components at the connectivity traced (the yardstick: README gives 2.4 ms for two labellings of such a map),
  - drs_polygon_count,
  - drs_polygon_rings at connectivity 4 and 8, the scratch sized for exactly the map's cracks,
  - drs_polygon_write into outputs sized exactly,
and of the whole loops.polygons (wall clock: it reads counters twice and copies the outputs to the host).  Each arm is launched
`warmup` times untimed, then `reps` times, one event pair per launch; the median and the extremes are reported, the arms interleaved.
Recorded beside the times: cracks, rings, holes, vertices, the longest ring, the rounds the two doublings ran (of the
ceil(log2(cracks)) and ceil(log2(cracks)) + 1 launched) and the scratch's size.  Prints one JSON line and writes it to out=.

    python tools/bench_polygons.py [mosaic=6000] [speckle=0.15] [min_size=64] [reps=7] [warmup=2] [out=profiles/polygons/cost.json]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_sieve import K, speckled_map  # noqa: E402
from drs_amd import _lib, loops  # noqa: E402

DEV = "cuda:0"
OPTIONS = ("mosaic", "speckle", "min_size", "reps", "warmup", "out")


def measure(name, m, n, reps, warmup):
    st = torch.cuda.current_stream(DEV).cuda_stream
    label = torch.empty((n, n), dtype=torch.int32, device=DEV)
    size = torch.empty((n, n), dtype=torch.int32, device=DEV)
    counters = torch.zeros(4, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.call("drs_polygon_count", m.data_ptr(), n, n, counters.data_ptr(), st)
    cracks = int(counters[0].item())
    nbytes = _lib.query("drs_polygon_scratch_bytes", n, n, cracks)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    facts, outs = {}, {}
    for c in (4, 8):
        _lib.call("drs_components", m.data_ptr(), n, n, c, label.data_ptr(), size.data_ptr(), st)
        _lib.call("drs_polygon_rings", m.data_ptr(), label.data_ptr(), n, n, c, cracks, scratch.data_ptr(), counters.data_ptr(), st)
        got, rings, vertices, bad = [int(v) for v in counters.cpu().tolist()]
        assert bad == 0 and got == cracks
        outs[c] = (torch.empty((rings, 7), dtype=torch.int64, device=DEV), torch.empty((vertices, 2), dtype=torch.int32, device=DEV))
        _lib.call("drs_polygon_write", scratch.data_ptr(), n, n, cracks, rings, vertices, outs[c][0].data_ptr(), outs[c][1].data_ptr(),
                  status.data_ptr(), st)
        assert int(status.item()) == 0
        head = scratch[:72].view(torch.int64).cpu().tolist()
        table = outs[c][0]
        facts["c%d" % c] = {"rings": rings, "holes": int((table[:, 6] < 0).sum().item()), "vertices": vertices,
                            "longest_ring_cracks": int(table[:, 5].max().item()),
                            "rounds_run": {"leaders": head[7], "ranks": head[8]},
                            "rounds_launched": {"leaders": (cracks - 1).bit_length(), "ranks": (cracks - 1).bit_length() + 1}}

    def components(c):
        _lib.call("drs_components", m.data_ptr(), n, n, c, label.data_ptr(), size.data_ptr(), st)

    def rings(c):
        _lib.call("drs_polygon_rings", m.data_ptr(), label.data_ptr(), n, n, c, cracks, scratch.data_ptr(), counters.data_ptr(), st)

    def write(c):
        _lib.call("drs_polygon_write", scratch.data_ptr(), n, n, cracks, outs[c][0].shape[0], outs[c][1].shape[0], outs[c][0].data_ptr(),
                  outs[c][1].data_ptr(), status.data_ptr(), st)

    arms = {"count": lambda: _lib.call("drs_polygon_count", m.data_ptr(), n, n, counters.data_ptr(), st)}
    for c in (4, 8):                               # components leaves the labels rings reads, rings the scratch write reads
        arms["components_c%d" % c] = lambda c=c: components(c)
        arms["rings_c%d" % c] = lambda c=c: rings(c)
        arms["write_c%d" % c] = lambda c=c: write(c)
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    del scratch, outs
    wall = {}
    for c in (4, 8):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loops.polygons(m, n, n, c)
            ts.append((time.perf_counter() - t0) * 1e3)
        wall["c%d" % c] = round(min(ts), 3)
    med = {k: statistics.median(t) for k, t in times.items()}
    return {"map": name, "cracks": cracks, "scratch_bytes": nbytes, "per_connectivity": facts,
            "arms_ms": {k: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for k, t in times.items()},
            "count_rings_write_ms": {"c%d" % c: round(med["count"] + med["rings_c%d" % c] + med["write_c%d" % c], 4) for c in (4, 8)},
            "over_components": {"c%d" % c: round((med["count"] + med["rings_c%d" % c] + med["write_c%d" % c]) / med["components_c%d" % c], 2)
                                for c in (4, 8)},
            "loops_polygons_wall_ms_best_of_3": wall}


def main(n, speckle, min_size, reps, warmup, out_path):
    assert torch.cuda.is_available(), "bench_polygons.py measures on the device: there is no CPU path"
    _lib.load()
    raw = speckled_map(n, speckle)
    sieved, info = loops.sieve_labels(raw, n, n, K, dict(min_size=min_size, connectivity=4))
    res = {"workload": "%dx%d speckled label map of K = %d (%g of the pixels re-drawn), sieved at min_size %d, connectivity 4 (%d rounds), "
                       "and unsieved" % (n, n, K, speckle, min_size, info["rounds"]),
           "reps": reps, "warmup": warmup,
           "maps": [measure("sieved", sieved, n, reps, warmup), measure("unsieved", raw, n, reps, warmup)],
           "device": torch.cuda.get_device_name(DEV)}
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    bad = [a for a in sys.argv[1:] if "=" not in a or a.split("=", 1)[0] not in OPTIONS]
    if bad:
        sys.exit("bench_polygons.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("mosaic", 6000)), float(kw.get("speckle", 0.15)), int(kw.get("min_size", 64)), int(kw.get("reps", 7)),
         int(kw.get("warmup", 2)), kw.get("out", os.path.join(ROOT, "profiles", "polygons", "cost.json")))
