#!/usr/bin/env python3
"""What the surface-distance scores (drs_distance_transform, drs_surface_histogram, loops.surface_histogram) cost, in
one process on one device, on the synthetic (truth, prediction) pair of tools/bench_objects.py (`mosaic` x `mosaic`, K = 6, the
prediction = the truth with `speckle` of the pixels re-drawn, ignore lines in the truth).  HIP-event times of
  - drs_surface_histogram on scratch allocated once (the contours of both maps, then per class two transforms and a gather),
  - the whole loops.surface_histogram, its allocation of the scratch included,
  - one drs_distance_transform (the contour of class 0 in the truth),
  - drs_boundary_histogram at its default distances and the whole loops.object_table on the same pair: the existing whole-map integer
    kernels, the yardsticks for "cheap next to what validation already does",
each launched `warmup` times untimed, then `reps` times, one event pair per call; the median and the extremes are reported, the arms
interleaved so that a drift of the clocks meets all of them.  Beside the table's time stands the time the bytes its pass structure must
move would take at the measured HBM copy rate (FLOOR_BYTES per pixel and transform, see below).  Prints one JSON line and writes it to
out=.

    python tools/bench_surface.py [mosaic=6000] [speckle=0.08] [reps=9] [warmup=2] [out=profiles/surface_scores/bench.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_objects import DEV, IGNORE, K, pair  # noqa: E402
from drs_amd import _lib, loops, metrics as MT, patches as P  # noqa: E402

OPTIONS = ("mosaic", "speckle", "reps", "warmup", "out")
# bytes per pixel one transform of the table must move, stack traffic (data-dependent, 0..16) left out: sites in (map 1, contour flag 1)
# and g out (2); g in, out, in (6) down and up the columns; g in (2) and d2 out (4) along the rows; d2 in (4), contour flag and map
# in (2) in the gather: 22 bytes = 5.5 passes of 4 h w
FLOOR_BYTES = 22
HBM_BYTES_PER_S = 6.29e12                   # the measured copy rate of the device, not the 8 TB/s of its data sheet


def main(n, speckle, reps, warmup, out_path):
    assert torch.cuda.is_available(), "bench_surface.py measures on the device: there is no CPU path"
    _lib.load()
    truth, pred = pair(n, speckle)
    st = torch.cuda.current_stream(DEV).cuda_stream
    shape = (2, K, MT.SURFACE_BINS + 2)
    raw, whole = torch.zeros(shape, dtype=torch.int64, device=DEV), torch.zeros(shape, dtype=torch.int64, device=DEV)
    need, need_dt = _lib.query("drs_surface_scratch_bytes", n, n), _lib.query("drs_distance_scratch_bytes", n, n)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    d2 = torch.empty((n, n), dtype=torch.int32, device=DEV)
    bhist = torch.zeros((len(P.BOUNDARY_DEFAULT) + 1,) * 2 + (K, K), dtype=torch.int64, device=DEV)
    otable = torch.zeros((K, 4, 32), dtype=torch.int64, device=DEV)
    arms = {
        "surface_histogram": lambda: _lib.call("drs_surface_histogram", truth.data_ptr(), pred.data_ptr(), n, n, K, IGNORE, raw.data_ptr(),
                                               scratch.data_ptr(), need, st),
        "surface_histogram_whole": lambda: loops.surface_histogram(truth, pred, n, n, K, IGNORE, table=whole, stream=st),
        "distance_transform": lambda: _lib.call("drs_distance_transform", truth.data_ptr(), None, 0, n, n, 2, 0, d2.data_ptr(),
                                                scratch.data_ptr(), need_dt, st),
        "boundary_histogram_d8": lambda: loops.boundary_histogram(truth, pred, n, n, K, IGNORE, P.BOUNDARY_DEFAULT, hist=bhist, stream=st),
        "object_table_whole": lambda: loops.object_table(truth, pred, n, n, K, IGNORE, 4, table=otable),
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
    res = {"workload": "%dx%d synthetic pair, K = %d, prediction = truth with %g of the pixels re-drawn, ignore lines every 500 pixels"
                       % (n, n, K, speckle), "reps": reps, "warmup": warmup}
    for name, t in times.items():
        res[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    torch.cuda.synchronize()
    calls = warmup + reps
    one = raw.cpu().numpy() // calls
    assert (one * calls == raw.cpu().numpy()).all() and (whole.cpu().numpy() == raw.cpu().numpy()).all(), "the arms disagree on the table"
    scores = MT.surface_scores(one, P.SURFACE_DEFAULT)
    sited = one[:, :, :MT.SURFACE_BINS].sum(axis=2)
    transforms = 2 * int(((sited[0] > 0) & (sited[1] > 0)).sum())
    res["contour_pixels_truth"], res["contour_pixels_pred"] = int(scores["n_truth"].sum()), int(scores["n_pred"].sum())
    res["mean_assd"], res["mean_hd95"] = round(scores["mean_assd"], 6), round(scores["mean_hd95"], 6)
    res["mean_nsd"] = [round(v, 6) for v in scores["mean_nsd"]]
    res["transforms"] = transforms
    res["scratch_bytes"] = int(need)
    res["floor_bytes_per_pixel_and_transform"] = FLOOR_BYTES
    res["floor_ms_at_hbm_rate"] = round(transforms * FLOOR_BYTES * n * n / HBM_BYTES_PER_S * 1e3, 4)
    res["surface_histogram_over_floor"] = round(res["surface_histogram_ms"]["median"] / res["floor_ms_at_hbm_rate"], 2) if transforms else None
    res["surface_histogram_over_boundary_histogram"] = round(res["surface_histogram_ms"]["median"] / res["boundary_histogram_d8_ms"]["median"], 3)
    res["surface_histogram_over_object_table"] = round(res["surface_histogram_ms"]["median"] / res["object_table_whole_ms"]["median"], 3)
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
        sys.exit("bench_surface.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("mosaic", 6000)), float(kw.get("speckle", 0.08)), int(kw.get("reps", 9)), int(kw.get("warmup", 2)),
         kw.get("out", os.path.join(ROOT, "profiles", "surface_scores", "bench.json")))
