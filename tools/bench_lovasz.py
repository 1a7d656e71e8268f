#!/usr/bin/env python3
"""What the Lovasz-softmax term of the training loss (drs_patch_lovasz_grad, drs_classifier_loss_region,
drs_net_set_lovasz) costs, in one process on one device, at the headline step's shape (128 patches of 64 x 64, K = 6) and at one
rank's share of a 85 x 85 step (16 patches): HIP-event times of
  - the classifier's inference form into the logits (the pre-pass's first launch), drs_patch_lovasz_grad over them, over keys that
    are all equal (logits = NULL: every digit of every pass falls into one bin) and over keys that are all distinct, and the fused
    classifier (C = 256, training) with Dice coefficients (drs_classifier_loss_dice) and with the map (drs_classifier_loss_region),
    plain and with gamma = 2,
each launched `warmup` times untimed, then `reps` times, one event pair per launch, the arms interleaved so that a drift of the clocks
meets all of them; the median and the extremes are reported.  Then the whole training step of the headline net (dilated_grsl_rate8,
5 bands) with the option off and on (lam = 1.5), alternately, by event pairs around `steps` steps each: the share of the step the
option costs ("off" is the same build with the option unset: launch for launch the step without this option); and the engine's own
timing kind "classifier_loss" per step, off and on.  Prints one JSON line and writes it to out=.

    python tools/bench_lovasz.py [shapes=128x64,16x85] [reps=15] [warmup=3] [steps=10] [rounds=5] [out=profiles/lovasz/cost.json]"""
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
LAM = 1.5
DICE = (1.0, 0.5, 0.5, 1.0)
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
    rows = _lib.query("drs_classifier_rows", B, S)
    gfeat = torch.empty(M * C, device=DEV)
    logits = torch.empty(M * K, device=DEV)
    pred = torch.empty(M, dtype=torch.uint8, device=DEV)
    dwp, dbp = torch.empty(rows * C * K, device=DEV), torch.empty(rows * K, device=DEV)
    lp = torch.empty(rows, dtype=torch.float64, device=DEV)
    conf = torch.zeros(K * K, dtype=torch.int32, device=DEV)
    coef = torch.zeros(B * K * 2, device=DEV)
    ploss = torch.zeros(B, dtype=torch.float64, device=DEV)
    err = torch.empty(M * K, device=DEV)
    region = torch.empty(M * K, device=DEV)
    lloss = torch.zeros(B, dtype=torch.float64, device=DEV)
    nbytes = _lib.query("drs_lovasz_scratch_bytes", B, S, K)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    equal = torch.full((M * K,), 0.5, device=DEV)
    # all distinct inside every (patch, class): a permutation of i / (S S) per patch
    perm = torch.stack([torch.randperm(S * S, device=DEV, generator=g) for _ in range(B)]).to(torch.float32) / float(S * S)
    distinct = perm.view(B, S * S, 1).expand(B, S * S, K).contiguous().view(-1)

    def infer():
        _lib.call("drs_classifier_loss_pixel", feat.data_ptr(), B, S, 0, C, 0, C, K, w.data_ptr(), b.data_ptr(), None, None, None, 1.0, None, 0.0,
                  None, logits.data_ptr(), None, None, 0, 0, None, None, None, None, st)

    def prepass(keys):
        lg, e = (logits.data_ptr(), err.data_ptr()) if keys is None else (None, keys.data_ptr())
        return lambda: _lib.call("drs_patch_lovasz_grad", lg, e, lab.data_ptr(), None, B, S, K, LAM, None, None, region.data_ptr(), lloss.data_ptr(),
                                 scratch.data_ptr(), nbytes, st)

    def cls(gamma, entry, extra):
        head = (feat.data_ptr(), B, S, 0, C, 0, C, K, w.data_ptr(), b.data_ptr(), lab.data_ptr(), None, valid.data_ptr(), 1.0 / M, None, gamma, None)
        tail = (None, pred.data_ptr(), gfeat.data_ptr(), C, 0, dwp.data_ptr(), dbp.data_ptr(), lp.data_ptr(), conf.data_ptr(), st)
        return lambda: _lib.call(entry, *(head + (extra.data_ptr(),) + tail))
    infer()
    _lib.call("drs_patch_dice_coeffs", logits.data_ptr(), lab.data_ptr(), None, B, S, K, *DICE, None, coef.data_ptr(), ploss.data_ptr(), st)
    arms = {"classifier_inference_logits": infer, "lovasz_grad": prepass(None), "lovasz_grad_all_ties": prepass(equal),
            "lovasz_grad_all_distinct": prepass(distinct)}
    res = {"workload": "%d patches of %d x %d, K = %d; classifier C = %d, training" % (B, S, S, K, C), "reps": reps, "warmup": warmup, "lam": LAM,
           "scratch_bytes": nbytes}
    res.update(timed(arms, reps, warmup))
    prepass(None)()
    torch.cuda.synchronize()
    arms = {"classifier_plain_dice": cls(0.0, "drs_classifier_loss_dice", coef), "classifier_plain_region": cls(0.0, "drs_classifier_loss_region", region),
            "classifier_focal_dice": cls(2.0, "drs_classifier_loss_dice", coef), "classifier_focal_region": cls(2.0, "drs_classifier_loss_region", region)}
    res.update(timed(arms, reps, warmup))
    del feat, gfeat
    # the whole step, option off and on, alternately
    from drs_amd.net import DilatedNet
    net = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=42)
    rng = np.random.default_rng(0)
    x = rng.normal(size=(B, S * S * CH)).astype(np.float32)
    net.feed(x, lab.cpu().numpy().reshape(B, -1), S, acc_mask=valid.cpu().numpy().reshape(B, -1))
    step_ms = {"off": [], "on": []}
    for r in range(rounds + 1):
        for name, lam in (("off", None), ("on", LAM)):
            net.set_lovasz(lam)
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
    for name, lam in (("off", None), ("on", LAM)):
        net.set_lovasz(lam)
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
    assert torch.cuda.is_available(), "bench_lovasz.py measures on the device: there is no CPU path"
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
        sys.exit("bench_lovasz.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main([tuple(int(v) for v in s.split("x")) for s in kw.get("shapes", "128x64,16x85").split(",")], int(kw.get("reps", 15)), int(kw.get("warmup", 3)),
         int(kw.get("steps", 10)), int(kw.get("rounds", 5)), kw.get("out", os.path.join(ROOT, "profiles", "lovasz", "cost.json")))
