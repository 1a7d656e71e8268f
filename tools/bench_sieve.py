#!/usr/bin/env python3
"""What the sieve (drs_components, drs_sieve_round, loops.sieve_labels) costs, in one process on one device: a
synthetic speckled label map (`mosaic` x `mosaic`, K = 6: Voronoi cells about mosaic / 20 pixels across with `speckle` of the pixels
re-drawn uniformly -- the shape of a noisy prediction), and HIP-event times of
  - drs_components at connectivity 4 and 8,
  - one drs_sieve_round (the first round of the map, out of place) at min_size,
  - drs_component_census,
  - drs_boundary_histogram at its default distances on (map, map): the existing whole-map integer kernel, the yardstick for "cheap
    next to what validation already does", and
  - a device-to-device copy of the map,
each launched `warmup` times untimed, then `reps` times, one event pair per launch; the median and the extremes are reported, the
arms interleaved so that a drift of the clocks meets all of them.  Then the whole loops.sieve_labels, host reads included, by the
wall clock around a synchronised call, with its info.  Prints one JSON line and writes it to out=.

    python tools/bench_sieve.py [mosaic=6000] [min_size=64] [speckle=0.15] [reps=9] [warmup=2] [out=profiles/sieve/bench.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drs_amd import _lib, loops, patches as P  # noqa: E402

DEV = "cuda:0"
K = 6
OPTIONS = ("mosaic", "min_size", "speckle", "reps", "warmup", "out")


def speckled_map(n, speckle, seed=0, cells=400):
    """uint8 [n][n] on the device: Voronoi cells of `cells` seeds, made on the device in row bands, then `speckle` of the pixels
    re-drawn uniformly from 0..K-1"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pts = torch.randint(0, n, (cells, 2), generator=g).float().to(DEV)
    labels = (torch.randperm(cells, generator=g) % K).to(torch.uint8).to(DEV)
    xs = torch.arange(n, device=DEV, dtype=torch.float32)
    out = torch.empty((n, n), dtype=torch.uint8, device=DEV)
    for y0 in range(0, n, 64):
        ys = torch.arange(y0, min(n, y0 + 64), device=DEV, dtype=torch.float32)
        d = (ys[:, None, None] - pts[None, None, :, 0]) ** 2 + (xs[None, :, None] - pts[None, None, :, 1]) ** 2
        out[y0:y0 + len(ys)] = labels[d.argmin(dim=-1)]
    g2 = torch.Generator(device=DEV).manual_seed(seed + 1)
    hit = torch.rand((n, n), generator=g2, device=DEV) < speckle
    out[hit] = torch.randint(0, K, (int(hit.sum().item()),), generator=g2, device=DEV).to(torch.uint8)
    return out.contiguous()


def main(n, min_size, speckle, reps, warmup, out_path):
    assert torch.cuda.is_available(), "bench_sieve.py measures on the device: there is no CPU path"
    _lib.load()
    m = speckled_map(n, speckle)
    st = torch.cuda.current_stream(DEV).cuda_stream
    label = {c: torch.empty(n * n, dtype=torch.int32, device=DEV) for c in (4, 8)}
    size = {c: torch.empty(n * n, dtype=torch.int32, device=DEV) for c in (4, 8)}
    scratch = torch.empty(_lib.query("drs_sieve_scratch_bytes", n, n) // 8, dtype=torch.int64, device=DEV)
    out = torch.empty_like(m)
    copy = torch.empty_like(m)
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    table = torch.zeros((K, 32), dtype=torch.int64, device=DEV)
    bhist = torch.zeros((len(P.BOUNDARY_DEFAULT) + 1,) * 2 + (K, K), dtype=torch.int64, device=DEV)
    ms = (ctypes.c_int * K)(*([min_size] * K))
    arms = {
        "components_4": lambda: _lib.call("drs_components", m.data_ptr(), n, n, 4, label[4].data_ptr(), size[4].data_ptr(), st),
        "components_8": lambda: _lib.call("drs_components", m.data_ptr(), n, n, 8, label[8].data_ptr(), size[8].data_ptr(), st),
        "sieve_round": lambda: _lib.call("drs_sieve_round", m.data_ptr(), label[4].data_ptr(), size[4].data_ptr(), n, n, K, ctypes.addressof(ms),
                                         scratch.data_ptr(), out.data_ptr(), counters.data_ptr(), st),
        "census": lambda: _lib.call("drs_component_census", m.data_ptr(), label[4].data_ptr(), size[4].data_ptr(), n, n, K, table.data_ptr(), st),
        "boundary_histogram_d8": lambda: loops.boundary_histogram(m, m, n, n, K, -1, P.BOUNDARY_DEFAULT, hist=bhist, stream=st),
        "copy_map": lambda: copy.copy_(m),
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
    res = {"workload": "%dx%d synthetic speckled map, K = %d, %g of the pixels re-drawn, min_size %d for every class" % (n, n, K, speckle, min_size),
           "reps": reps, "warmup": warmup}
    for name, t in times.items():
        res[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    small, merged = counters.cpu().tolist()
    res["first_round_small_components"], res["first_round_merged"] = int(small), int(merged)
    res["components_4_count"] = int((label[4] == torch.arange(n * n, dtype=torch.int32, device=DEV)).sum().item())
    res["components_8_count"] = int((label[8] == torch.arange(n * n, dtype=torch.int32, device=DEV)).sum().item())
    res["largest_component_4"] = int(size[4].max().item())
    for c in (4, 8):
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sieved, info = loops.sieve_labels(m, n, n, K, dict(min_size=min_size, connectivity=c))
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        res["sieve_labels_%d_wall_ms" % c] = {"median": round(statistics.median(walls), 3), "min": round(min(walls), 3), "max": round(max(walls), 3)}
        res["sieve_labels_%d_info" % c] = info
    res["components_4_over_boundary_histogram"] = round(res["components_4_ms"]["median"] / res["boundary_histogram_d8_ms"]["median"], 3)
    res["sieve_round_over_boundary_histogram"] = round(res["sieve_round_ms"]["median"] / res["boundary_histogram_d8_ms"]["median"], 3)
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
        sys.exit("bench_sieve.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("mosaic", 6000)), int(kw.get("min_size", 64)), float(kw.get("speckle", 0.15)), int(kw.get("reps", 9)),
         int(kw.get("warmup", 2)), kw.get("out", os.path.join(ROOT, "profiles", "sieve", "bench.json")))
