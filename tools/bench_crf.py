#!/usr/bin/env python3
"""What the local dense-CRF refinement costs next to the inference it refines, in one process: on bench_dense_predict's
6000 x 6000 x 5 synthetic mosaic (BASELINE config 5: Dilated8Pooling, tiles of 512), `reps` alternating runs of overlap-tile inference
with return_sums=True and of loops.refine_crf at the defaults on those sums (5 iterations, radius 5, step 2: 120 neighbours per pixel
and iteration), each timed by HIP events on the launch stream; then `reps` timings of one drs_crf_step launch alone.  Prints one JSON
line and writes it to out= (default profiles/crf_refine/bench.json) with the clocks the device reports before and after, the ratio of
refinement to inference and the neighbour visits per second of the step kernel.

    python tools/bench_crf.py [mosaic=6000] [tile=512] [reps=3] [out=profiles/crf_refine/bench.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_dense_predict import K, NET, setup  # noqa: E402
from drs_amd import _lib, loops, patches as P  # noqa: E402

DEV = "cuda:0"
OPTIONS = ("mosaic", "tile", "reps", "out")


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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, out


def main(mosaic, tile, reps, out_path):
    dev, n, S, Bw, pool, net, mean, std, nh, nw, allpos = setup(NET, mosaic)
    T = min(n, tile)
    boxes = P.dense_tiles(n, n, T, *net.plan.receptive_field)
    B_t = loops.dense_batch(net.plan, T)
    twin = loops.dense_twin(net, T, B_t)
    for b in sorted({B_t, len(boxes) % B_t} - {0}):          # every shape the inference launches, code objects loaded outside the timing
        P.crop_to_net(twin, pool, np.concatenate([np.zeros((b, 1), dtype=np.int64), boxes[:b, :2]], axis=1), T, mean, std)
        twin.forward(b, T)
    crf = P.check_crf(True)
    path = loops.InferencePath(dense_tile=T)
    comm = loops.NoComm()

    def infer():
        return path.run(net, pool, 0, B_t, mean, std, comm, return_sums=True)
    sums, occur, is_prob = infer()
    loops.refine_crf(net, pool, 0, sums, occur, is_prob, 1)          # one iteration: loads the code objects
    torch.cuda.synchronize()
    before = clocks()
    t_inf, t_crf = [], []
    for _ in range(reps):
        t, (sums, occur, is_prob) = timed(infer)
        t_inf.append(round(t, 4))
        t, (labels, _) = timed(lambda: loops.refine_crf(net, pool, 0, sums, occur, is_prob, crf))
        t_crf.append(round(t, 4))
    # one step alone, on buffers of its own
    npix = n * n
    logp = torch.empty(npix * K, dtype=torch.float32, device=dev)
    q = [torch.empty(npix * K, dtype=torch.float32, device=dev) for _ in range(2)]
    live = torch.empty(npix, dtype=torch.int32, device=dev)
    st = net._stream()
    _lib.call("drs_crf_unary", sums.data_ptr(), occur.data_ptr(), n, n, K, 0, 1.0, logp.data_ptr(), q[0].data_ptr(), live.data_ptr(), st)
    tile_ptr = pool.tiles.data_ptr()

    def step():
        _lib.call("drs_crf_step", q[0].data_ptr(), logp.data_ptr(), live.data_ptr(), tile_ptr, 1 if pool.f64 else 0, pool.C, n, n, K, 0, n,
                  crf.radius, crf.step, crf.w_app, crf.theta_xy, crf.theta_rgb, crf.w_smooth, crf.theta_s, q[1].data_ptr(), st)
    step()
    t_step = [round(timed(step)[0], 5) for _ in range(reps)]
    visits = npix * ((2 * crf.radius + 1) ** 2 - 1)
    best_inf, best_crf, best_step = min(t_inf), min(t_crf), min(t_step)
    res = {"workload": "%dx%dx%d synthetic mosaic, %s, overlap-tile inference at T = %d with return_sums against loops.refine_crf at "
                       "the defaults %s" % (n, n, pool.C, NET, T, tuple(crf)),
           "reps": reps, "inference_s": t_inf, "refine_crf_s": t_crf, "one_step_s": t_step,
           "refine_over_inference": round(best_crf / best_inf, 4), "steps_share_of_refine": round(crf.iters * best_step / best_crf, 4),
           "neighbours_per_pixel": (2 * crf.radius + 1) ** 2 - 1, "neighbour_visits_per_step": visits,
           "neighbour_visits_per_s": round(visits / best_step, 1), "labels_checksum": int(labels.long().sum().item()),
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
        sys.exit("bench_crf.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("mosaic", 6000)), int(kw.get("tile", 512)), int(kw.get("reps", 3)),
         kw.get("out", os.path.join(ROOT, "profiles", "crf_refine", "bench.json")))
