#!/usr/bin/env python3
"""What the superpixel vote (drs_superpixel_features, drs_superpixels, drs_components on the colouring,
drs_region_vote) costs, in one process on one device: a synthetic `mosaic` x `mosaic` x 5 fp32 image (blocks of random colour about
24 pixels across under noise -- roofs and roads under texture), a speckled label map of K = 6 (tools/bench_sieve.py's) and a random
confidence map, and HIP-event times, at every grid step in `sizes`, of
  - drs_superpixel_features,
  - drs_superpixels at 1 iteration and at `iters` iterations: one iteration (the assignment launch, which also sums per centre, and
    the launch of the means) costs the difference over iters - 1, the start the rest,
  - drs_components at connectivity 4 on the 16-colouring,
  - drs_region_vote without weights and with the confidence map,
and, once, of `iters` drs_crf_step launches at the CRF's defaults on the same image -- the neighbour a user chooses against -- and of
a device-to-device copy of the image.  Each arm is launched `warmup` times untimed, then `reps` times, one event pair per launch; the
median and the extremes are reported, the arms interleaved so that a drift of the clocks meets all of them.  Beside each time: the
bytes the stage must move (computed from the shapes, below) and the time that would take at the measured HBM copy rate.  The two
launches of an iteration are told apart only by a kernel trace: `kernel_stats=` names the kernel statistics CSV of a run of this same
command under `rocprofv3 --kernel-trace --stats` (a run of its own), whose per-kernel averages are then copied into the result.
Prints one JSON line and writes it to out=.

    python tools/bench_superpixels.py [mosaic=6000] [sizes=8,16] [iters=5] [reps=7] [warmup=2] [kernel_stats=] [out=profiles/superpixels/cost.json]"""
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_sieve import speckled_map  # noqa: E402
from drs_amd import _lib, patches as P  # noqa: E402

DEV = "cuda:0"
K, C = 6, 5
HBM_BYTES_PER_S = 6.29e12                   # the measured copy rate of the device (tools/bench_surface.py), not the 8 TB/s of its data sheet
OPTIONS = ("mosaic", "sizes", "iters", "reps", "warmup", "kernel_stats", "out")
KERNELS = ("sp_features_kernel", "sp_init_kernel", "sp_assign_kernel", "sp_update_kernel", "cc_local_kernel", "cc_merge_kernel",
           "cc_flatten_kernel", "cc_spread_kernel", "vote_init_kernel", "vote_add_kernel", "vote_best_kernel", "vote_apply_kernel",
           "crf_step_kernel")


def image(n, seed=0, block=24):
    """fp32 [n][n][C] on the device: random colours per block of `block` pixels plus 4 % uniform noise"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    nb = n // block + 2
    coarse = torch.rand((nb, nb, C), generator=g, device=DEV)
    idx = torch.arange(n, device=DEV) // block
    out = coarse[idx][:, idx].contiguous()
    out += 0.04 * torch.rand((n, n, C), generator=g, device=DEV)
    return out.contiguous()


def floors(n, S, iters):
    """the bytes each stage must move, from the shapes: per pixel unless said otherwise"""
    px, nc = n * n, max(1, n // S) ** 2
    centre = 4 * (C + 3)
    return {
        "features": px * (4 * C + C),                                  # the fp32 image in, the bytes out
        "assign": px * (C + 4 + 1) + nc * 2 * centre,                  # features in, assign and colour out; centres in, sums out
        "update": nc * 3 * centre,                                     # sums in, centres and zeroed sums out
        "components": px * (1 + 4 + 4),                                # colour in, label and size out
        "vote": px * (1 + 4 + 1),                                      # map and labels in, map out: once, whatever K
        "vote_weighted": px * (1 + 4 + 1 + 1),
        "crf_steps": iters * px * (2 * 4 * K + 4 * K + 4 + 4 * C),     # per step Q in and out, the unary, live, the image
        "copy_image": px * 2 * 4 * C,
    }


def kernel_averages(path):
    """{kernel: {"calls", "average_ms"}} of the kernels of these stages from a rocprofv3 kernel statistics CSV"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name in KERNELS:
                if name in row["Name"]:
                    cur = out.setdefault(name, {"calls": 0, "total_ms": 0.0})
                    cur["calls"] += int(row["Calls"])
                    cur["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    return {k: {"calls": v["calls"], "average_ms": round(v["total_ms"] / v["calls"], 4)} for k, v in out.items()}


def main(n, sizes, iters, reps, warmup, stats_path, out_path):
    assert torch.cuda.is_available(), "bench_superpixels.py measures on the device: there is no CPU path"
    _lib.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    img = image(n)
    pred = speckled_map(n, 0.15)
    g = torch.Generator(device=DEV).manual_seed(5)
    conf = torch.randint(0, 256, (n, n), generator=g, device=DEV, dtype=torch.uint8)
    lo, hi = torch.aminmax(img.view(n * n, C), dim=0)
    lo, hi = lo.cpu().numpy().astype(np.float32), hi.cpu().numpy().astype(np.float32)
    inv = (np.float32(255) / (hi - lo)).astype(np.float32)
    feat = torch.empty((n, n, C), dtype=torch.uint8, device=DEV)
    assign = torch.empty((n, n), dtype=torch.int32, device=DEV)
    colour = torch.empty((n, n), dtype=torch.uint8, device=DEV)
    label = torch.empty((n, n), dtype=torch.int32, device=DEV)
    size = torch.empty((n, n), dtype=torch.int32, device=DEV)
    out = torch.empty_like(pred)
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    vscratch = torch.empty(_lib.query("drs_region_vote_scratch_bytes", n, n) // 8, dtype=torch.int64, device=DEV)
    copy = torch.empty_like(img)
    bufs = {}
    for S in sizes:
        need = _lib.query("drs_superpixel_scratch_bytes", C, n, n, S)
        bufs[S] = (torch.empty(need // 4, dtype=torch.int32, device=DEV), torch.empty(need // 4, dtype=torch.int32, device=DEV))

    def slic(S, it):
        centres, scratch = bufs[S]
        _lib.call("drs_superpixels", feat.data_ptr(), C, n, n, S, P.SUPERPIXEL_DEFAULTS.compactness, it, assign.data_ptr(), colour.data_ptr(),
                  centres.data_ptr(), scratch.data_ptr(), st)

    def vote(weight):
        _lib.call("drs_region_vote", pred.data_ptr(), label.data_ptr(), None if weight is None else weight.data_ptr(), n, n, K,
                  vscratch.data_ptr(), out.data_ptr(), counters.data_ptr(), st)

    # the CRF's buffers: a random posterior, every pixel covered
    crf = P.check_crf(True)
    sums = torch.randn(n * n * K, generator=g, device=DEV, dtype=torch.float32)
    occur = torch.ones(n * n, dtype=torch.int32, device=DEV)
    logp = torch.empty(n * n * K, dtype=torch.float32, device=DEV)
    q = [torch.empty(n * n * K, dtype=torch.float32, device=DEV) for _ in range(2)]
    live = torch.empty(n * n, dtype=torch.int32, device=DEV)
    _lib.call("drs_crf_unary", sums.data_ptr(), occur.data_ptr(), n, n, K, 0, 1.0, logp.data_ptr(), q[0].data_ptr(), live.data_ptr(), st)
    del sums

    def crf_steps():
        for it in range(iters):
            _lib.call("drs_crf_step", q[it & 1].data_ptr(), logp.data_ptr(), live.data_ptr(), img.data_ptr(), 0, C, n, n, K, 0, n, crf.radius,
                      crf.step, crf.w_app, crf.theta_xy, crf.theta_rgb, crf.w_smooth, crf.theta_s, q[(it + 1) & 1].data_ptr(), st)

    arms = {"features": lambda: _lib.call("drs_superpixel_features", img.data_ptr(), 0, C, n, n, lo.ctypes.data, inv.ctypes.data,
                                          feat.data_ptr(), st)}
    for S in sizes:
        arms["superpixels_1_S%d" % S] = lambda S=S: slic(S, 1)
        arms["superpixels_%d_S%d" % (iters, S)] = lambda S=S: slic(S, iters)      # leaves the colouring the next three arms read
        arms["components_S%d" % S] = lambda: _lib.call("drs_components", colour.data_ptr(), n, n, 4, label.data_ptr(), size.data_ptr(), st)
        arms["vote_S%d" % S] = lambda: vote(None)
        arms["vote_weighted_S%d" % S] = lambda: vote(conf)
    arms["crf_steps"] = crf_steps
    arms["copy_image"] = lambda: copy.copy_(img)
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    facts = {}
    for rep in range(reps):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
            if rep == 0 and name.startswith("vote_S"):
                S = int(name[6:])
                regions, changed = [int(v) for v in counters.cpu().tolist()]
                facts["S%d" % S] = {"centres": max(1, n // S) ** 2, "regions": regions, "changed_pixels": changed,
                                    "largest_region": int(size.max().item())}
    med = {name: statistics.median(t) for name, t in times.items()}
    res = {"workload": "%dx%dx%d synthetic fp32 image (random blocks of 24 pixels under noise), speckled label map of K = %d, compactness %d, "
                       "%d iterations" % (n, n, C, K, P.SUPERPIXEL_DEFAULTS.compactness, iters),
           "reps": reps, "warmup": warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "note": "the assignment launch also sums per centre (LDS, then global integer atomics); 'update' is the launch of the means",
           "arms_ms": {name: {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for name, t in times.items()}}
    stages = {}
    for S in sizes:
        fl = floors(n, S, iters)
        per_iter = (med["superpixels_%d_S%d" % (iters, S)] - med["superpixels_1_S%d" % S]) / max(1, iters - 1)
        rows = {"features": med["features"], "iteration_assign_plus_update": per_iter,
                "start": med["superpixels_1_S%d" % S] - per_iter, "superpixels_all_iterations": med["superpixels_%d_S%d" % (iters, S)],
                "components": med["components_S%d" % S], "vote": med["vote_S%d" % S], "vote_weighted": med["vote_weighted_S%d" % S]}
        floor_of = {"features": fl["features"], "iteration_assign_plus_update": fl["assign"] + fl["update"],
                    "superpixels_all_iterations": iters * (fl["assign"] + fl["update"]), "components": fl["components"], "vote": fl["vote"],
                    "vote_weighted": fl["vote_weighted"]}
        total = med["features"] + med["superpixels_%d_S%d" % (iters, S)] + med["components_S%d" % S] + med["vote_S%d" % S]
        stages["S%d" % S] = dict(facts.get("S%d" % S, {}), whole_vote_ms=round(total, 4),
                                 whole_vote_over_crf_steps=round(total / med["crf_steps"], 4),
                                 stages={k: dict(ms=round(v, 4), **({"bytes": floor_of[k], "floor_ms_at_hbm_rate": round(floor_of[k] / HBM_BYTES_PER_S * 1e3, 4)}
                                                                     if k in floor_of else {})) for k, v in rows.items()})
    res["per_size"] = stages
    fl = floors(n, sizes[0], iters)
    res["crf_steps"] = {"iters": iters, "params": list(crf), "ms": round(med["crf_steps"], 4), "bytes": fl["crf_steps"],
                        "floor_ms_at_hbm_rate": round(fl["crf_steps"] / HBM_BYTES_PER_S * 1e3, 4)}
    res["copy_image"] = {"ms": round(med["copy_image"], 4), "bytes": fl["copy_image"],
                         "bytes_per_s": round(fl["copy_image"] / (med["copy_image"] / 1e3), 1)}
    if stats_path:
        res["kernel_averages_from_trace"] = kernel_averages(stats_path)
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
        sys.exit("bench_superpixels.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("mosaic", 6000)), [int(s) for s in kw.get("sizes", "8,16").split(",")], int(kw.get("iters", 5)), int(kw.get("reps", 7)),
         int(kw.get("warmup", 2)), kw.get("kernel_stats", ""), kw.get("out", os.path.join(ROOT, "profiles", "superpixels", "cost.json")))
