#!/usr/bin/env python3
"""What the object scores (drs_object_match, drs_object_table, loops.object_table) cost, in one process on one device:
a synthetic (truth, prediction) pair (`mosaic` x `mosaic`, K = 6: Voronoi cells about mosaic / 20 pixels across; the prediction is the
truth with `speckle` of the pixels re-drawn uniformly -- the shape of a noisy prediction -- and the truth carries a grid of lines of
the ignore label, as the ISPRS noBoundary ground truth does), and HIP-event times of
  - the whole loops.object_table (two drs_components, drs_object_match, drs_object_table, its allocations included),
  - the two drs_components calls alone,
  - drs_object_match alone (its four launches) and drs_object_table alone,
  - drs_boundary_histogram at its default distances on the same pair: the existing whole-map integer kernel, the yardstick for "cheap
    next to what validation already does",
each launched `warmup` times untimed, then `reps` times, one event pair per call; the median and the extremes are reported, the arms
interleaved so that a drift of the clocks meets all of them.  Prints one JSON line and writes it to out=.

    python tools/bench_objects.py [mosaic=6000] [speckle=0.08] [connectivity=4] [reps=9] [warmup=2] [out=profiles/object_scores/bench.json]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drs_amd import _lib, loops, metrics as MT, patches as P  # noqa: E402

DEV = "cuda:0"
K = 6
IGNORE = 6
OPTIONS = ("mosaic", "speckle", "connectivity", "reps", "warmup", "out")


def pair(n, speckle, seed=0, cells=400):
    """(truth, pred) uint8 [n][n] on the device: Voronoi cells of `cells` seeds, made on the device in row bands; pred = the cells with
    `speckle` of the pixels re-drawn uniformly from 0..K-1; truth = the cells with every 500th row and column set to the ignore label"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pts = torch.randint(0, n, (cells, 2), generator=g).float().to(DEV)
    labels = (torch.randperm(cells, generator=g) % K).to(torch.uint8).to(DEV)
    xs = torch.arange(n, device=DEV, dtype=torch.float32)
    truth = torch.empty((n, n), dtype=torch.uint8, device=DEV)
    for y0 in range(0, n, 64):
        ys = torch.arange(y0, min(n, y0 + 64), device=DEV, dtype=torch.float32)
        d = (ys[:, None, None] - pts[None, None, :, 0]) ** 2 + (xs[None, :, None] - pts[None, None, :, 1]) ** 2
        truth[y0:y0 + len(ys)] = labels[d.argmin(dim=-1)]
    pred = truth.clone()
    g2 = torch.Generator(device=DEV).manual_seed(seed + 1)
    hit = torch.rand((n, n), generator=g2, device=DEV) < speckle
    pred[hit] = torch.randint(0, K, (int(hit.sum().item()),), generator=g2, device=DEV).to(torch.uint8)
    truth[::500] = IGNORE
    truth[:, ::500] = IGNORE
    return truth.contiguous(), pred.contiguous()


def main(n, speckle, c, reps, warmup, out_path):
    assert torch.cuda.is_available(), "bench_objects.py measures on the device: there is no CPU path"
    _lib.load()
    truth, pred = pair(n, speckle)
    st = torch.cuda.current_stream(DEV).cuda_stream
    tlabel, tsize, plabel, psize, match, inter, cover = [torch.empty(n * n, dtype=torch.int32, device=DEV) for _ in range(7)]
    scratch = torch.empty(_lib.query("drs_object_scratch_bytes", n, n) // 8, dtype=torch.int64, device=DEV)
    table = torch.zeros((K, 4, 32), dtype=torch.int64, device=DEV)
    whole = torch.zeros((K, 4, 32), dtype=torch.int64, device=DEV)
    bhist = torch.zeros((len(P.BOUNDARY_DEFAULT) + 1,) * 2 + (K, K), dtype=torch.int64, device=DEV)

    def two_components():
        _lib.call("drs_components", truth.data_ptr(), n, n, c, tlabel.data_ptr(), tsize.data_ptr(), st)
        _lib.call("drs_components", pred.data_ptr(), n, n, c, plabel.data_ptr(), psize.data_ptr(), st)
    arms = {
        "object_table_whole": lambda: loops.object_table(truth, pred, n, n, K, IGNORE, c, table=whole),
        "two_components": two_components,
        "object_match": lambda: _lib.call("drs_object_match", truth.data_ptr(), pred.data_ptr(), tlabel.data_ptr(), tsize.data_ptr(),
                                          plabel.data_ptr(), psize.data_ptr(), n, n, K, IGNORE, scratch.data_ptr(), match.data_ptr(),
                                          inter.data_ptr(), cover.data_ptr(), st),
        "object_table": lambda: _lib.call("drs_object_table", truth.data_ptr(), tlabel.data_ptr(), tsize.data_ptr(), pred.data_ptr(),
                                          plabel.data_ptr(), psize.data_ptr(), match.data_ptr(), inter.data_ptr(), cover.data_ptr(), n, n, K,
                                          IGNORE, table.data_ptr(), st),
        "boundary_histogram_d8": lambda: loops.boundary_histogram(truth, pred, n, n, K, IGNORE, P.BOUNDARY_DEFAULT, hist=bhist, stream=st),
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
    res = {"workload": "%dx%d synthetic pair, K = %d, prediction = truth with %g of the pixels re-drawn, ignore lines every 500 pixels, "
                       "connectivity %d" % (n, n, K, speckle, c), "reps": reps, "warmup": warmup}
    for name, t in times.items():
        res[name + "_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    torch.cuda.synchronize()
    calls = warmup + reps
    one = (table.cpu().numpy() // calls)
    assert (one * calls == table.cpu().numpy()).all() and (whole.cpu().numpy() == table.cpu().numpy()).all(), "the arms disagree on the table"
    scores = MT.object_scores(one)
    res["truth_objects"], res["predicted_objects"], res["matched"] = [int(scores["all"][k]) for k in ("truth", "predicted", "matched")]
    res["all_f1"], res["all_sq"], res["all_pq"] = [round(scores["all"][k], 6) for k in ("f1", "sq", "pq")]
    res["largest_truth_object"] = int(tsize.max().item())
    res["match_and_table_over_two_components"] = round((res["object_match_ms"]["median"] + res["object_table_ms"]["median"]) /
                                                       res["two_components_ms"]["median"], 3)
    res["whole_over_boundary_histogram"] = round(res["object_table_whole_ms"]["median"] / res["boundary_histogram_d8_ms"]["median"], 3)
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
        sys.exit("bench_objects.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("mosaic", 6000)), float(kw.get("speckle", 0.08)), int(kw.get("connectivity", 4)), int(kw.get("reps", 9)),
         int(kw.get("warmup", 2)), kw.get("out", os.path.join(ROOT, "profiles", "object_scores", "bench.json")))
