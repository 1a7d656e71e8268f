#!/usr/bin/env python3
"""What the boundary (surface) loss of the training loss (drs_patch_surface_loss, drs_net_set_surface_loss) costs, in
one process on one device, at the headline step's shape (128 patches of 64 x 64, K = 6) and at one rank's share of a 85 x 85 step
(16 patches): HIP-event times of
  - the classifier's inference form into the logits (the pre-passes' shared first launch) and drs_patch_surface_loss over them on
    three kinds of labels: blobs (the labels of the other cost tools), random speckle (every distance is a pixel or two: the row
    scan stops at once) and a patch with one lone pixel of each class (every other pixel scans its whole row: the scan's worst
    case),
each launched `warmup` times untimed, then `reps` times, one event pair per launch, the arms interleaved so that a drift of the clocks
meets all of them; the median and the extremes are reported.  Then the whole training step of the headline net (dilated_grsl_rate8,
5 bands) on the blob labels with the option off and on (lam = 0.5, clip 20), alternately, by event pairs around `steps` steps each:
the share of the step the option costs ("off" is the same build with the option unset: launch for launch the step without this
option); and the engine's own timing kind "classifier_loss" per step, off and on.  Prints one JSON line and writes it to out=.

    python tools/bench_surface_loss.py [shapes=128x64,16x85] [reps=15] [warmup=3] [steps=10] [rounds=5] [out=profiles/surface_loss/cost.json]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from drs_amd import _lib  # noqa: E402
from bench_boundary_weight import blob_labels, timed  # noqa: E402  (the same labels and the same interleaved timing)

DEV = "cuda:0"
K, C, CH, NET = 6, 256, 5, "dilated_grsl_rate8"
SURF = (0.5, 20.0)
OPTIONS = ("shapes", "reps", "warmup", "steps", "rounds", "out")


def one_shape(B, S, reps, warmup, steps, rounds):
    st = torch.cuda.current_stream(DEV).cuda_stream
    M = B * S * S
    lab, valid = blob_labels(B, S)
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    feat = torch.randn(M * C, device=DEV, generator=g)
    w = torch.randn(C * K, device=DEV, generator=g) / 16
    b = torch.zeros(K, device=DEV)
    logits = torch.empty(M * K, device=DEV)
    region = torch.empty(M * K, device=DEV)
    sloss = torch.zeros(B, dtype=torch.float64, device=DEV)
    nbytes = _lib.query("drs_surface_loss_scratch_bytes", B, S, K)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    speckle = torch.randint(0, K, (M,), device=DEV, generator=g).to(torch.uint8)
    lone = torch.zeros(B, S, S, dtype=torch.uint8, device=DEV)
    for c in range(1, K):                      # one pixel of each class 1 .. K - 1 along the top row, class 0 everywhere else
        lone[:, 0, (c - 1) * (S - 1) // max(1, K - 2)] = c
    lone = lone.view(-1).contiguous()

    def infer():
        _lib.call("drs_classifier_loss_pixel", feat.data_ptr(), B, S, 0, C, 0, C, K, w.data_ptr(), b.data_ptr(), None, None, None, 1.0, None, 0.0,
                  None, logits.data_ptr(), None, None, 0, 0, None, None, None, None, st)

    def prepass(labels, va):
        return lambda: _lib.call("drs_patch_surface_loss", logits.data_ptr(), labels.data_ptr(), None, None if va is None else va.data_ptr(), B, S, K,
                                 SURF[0], SURF[1], None, 0, None, region.data_ptr(), sloss.data_ptr(), scratch.data_ptr(), nbytes, st)
    infer()
    arms = {"classifier_inference_logits": infer, "surface_loss_blobs": prepass(lab, valid), "surface_loss_speckle": prepass(speckle, None),
            "surface_loss_lone_pixels": prepass(lone, None)}
    res = {"workload": "%d patches of %d x %d, K = %d" % (B, S, S, K), "reps": reps, "warmup": warmup, "lam": SURF[0], "clip": SURF[1],
           "scratch_bytes": nbytes}
    res.update(timed(arms, reps, warmup))
    del feat
    # the whole step, option off and on, alternately
    from drs_amd.net import DilatedNet
    net = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=42)
    rng = np.random.default_rng(0)
    x = rng.normal(size=(B, S * S * CH)).astype(np.float32)
    net.feed(x, lab.cpu().numpy().reshape(B, -1), S, acc_mask=valid.cpu().numpy().reshape(B, -1))
    step_ms = {"off": [], "on": []}
    for r in range(rounds + 1):
        for name, s in (("off", None), ("on", SURF)):
            net.set_surface_loss(s)
            net.train_step(B, S, 0.01)          # (the first step after a switch, untimed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                net.train_step(B, S, 0.01)
            e1.record()
            e1.synchronize()
            if r:                               # (round 0 is the warm-up)
                step_ms[name].append(e0.elapsed_time(e1) / steps)
    for name, t in step_ms.items():
        res["step_%s_ms" % name] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    off, on = res["step_off_ms"]["median"], res["step_on_ms"]["median"]
    res["step_on_minus_off_ms"] = round(on - off, 4)
    res["option_share_of_step"] = round((on - off) / off, 5)
    for name, s in (("off", None), ("on", SURF)):
        net.set_surface_loss(s)
        net.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        net.timer = True
        for _ in range(steps):
            net.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        kind = net.timer.summary()["classifier_loss"]
        net.timer = None
        res["engine_classifier_loss_kind_%s_ms_per_step" % name] = round(kind["ms"] / steps, 4)
    return res


def main(shapes, reps, warmup, steps, rounds, out_path):
    assert torch.cuda.is_available(), "bench_surface_loss.py measures on the device: there is no CPU path"
    _lib.load()
    res = {"%dx%dx%d" % (B, S, S): one_shape(B, S, reps, warmup, steps, rounds) for B, S in shapes}
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
        sys.exit("bench_surface_loss.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main([tuple(int(v) for v in s.split("x")) for s in kw.get("shapes", "128x64,16x85").split(",")], int(kw.get("reps", 15)), int(kw.get("warmup", 3)),
         int(kw.get("steps", 10)), int(kw.get("rounds", 5)), kw.get("out", os.path.join(ROOT, "profiles", "surface_loss", "cost.json")))
