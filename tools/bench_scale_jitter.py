#!/usr/bin/env python3
"""Cost of the training crop's scale jitter at the headline shape: Dilated8Pooling, 128 x 64 x 64 x 5, fp64 tiles, one
GPU.  A step here is what loops.train does per step: the augmentation draws (with the scale draws and the footprints when the option
is on), the crop -- drs_crop_normalize, or drs_crop_normalize_scaled with the option -- and drs_train_step.

  python tools/bench_scale_jitter.py [steps=60] [rounds=3] [jitter=0.75,1.25] [out=file.json]
      `rounds` alternating blocks of `steps` steps with the option off and on, ms per step of each block, their medians and the ratio
  python tools/bench_scale_jitter.py mode=off|on steps=10
      one arm only: the form to run under `rocprofv3 --kernel-trace --stats` (crop_kernel / crop_scaled_kernel beside the step's kernels)
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drs_amd import patches as P                                # noqa: E402
from drs_amd.net import DilatedNet                              # noqa: E402
from drs_amd.synthetic import grid_instances, make_tile         # noqa: E402

B, S, TILE = 128, 64, 2048


def main(steps=60, rounds=3, jitter=(0.75, 1.25), mode=None, out=None):
    dev = "cuda:0"
    tile, lab = make_tile(TILE, TILE, 5, 6, seed=1234)
    pool = P.TilePool([tile], [lab], dev)
    inst = grid_instances(TILE, TILE, S, 25, B * 100, seed=0)
    net = DilatedNet("dilated_grsl_rate8", 5, 6, 0.005, b_max=B, s_max=S, device=dev, seed=42)
    np.random.seed(0)
    count = [0]

    def step(on):
        i = count[0]
        count[0] += 1
        rows = inst[(i * B) % (B * 99):(i * B) % (B * 99) + B]
        aug = P.draw_augmentation(rows, S, 5, noise="device", scale_jitter=jitter if on else None, jitter_key=(7, i) if on else None)
        if on:
            aug.geo = P.scale_geometry(rows, pool, S, aug.scale)
        P.crop_to_net(net, pool, rows, S, [0.5] * 3, [0.2] * 3, aug)
        return net.train_step(B, S, 0.01)

    def block(on, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(on)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    if mode is not None:
        on = mode == "on"
        block(on, 5)
        print("%s: %.3f ms/step over %d steps" % (mode, block(on, steps), steps))
        return
    block(False, 5)
    block(True, 5)
    off, onn = [], []
    for _ in range(rounds):
        off.append(block(False, steps))
        onn.append(block(True, steps))
    res = dict(what="one training step at %d x %d x %d x 5 (dilated_grsl_rate8, fp64 tiles): host draws + crop + drs_train_step; %d alternating "
                    "blocks of %d steps per arm, ms per step" % (B, S, S, rounds, steps),
               jitter=list(jitter), off_ms=[round(v, 4) for v in off], on_ms=[round(v, 4) for v in onn],
               off_median_ms=round(float(np.median(off)), 4), on_median_ms=round(float(np.median(onn)), 4),
               on_over_off=round(float(np.median(onn) / np.median(off)), 5), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    kw = dict(a.split("=") for a in sys.argv[1:])
    main(int(kw.get("steps", 60)), int(kw.get("rounds", 3)), tuple(float(v) for v in kw.get("jitter", "0.75,1.25").split(",")),
         kw.get("mode"), kw.get("out"))
