#!/usr/bin/env python3
"""What the soft Dice / Tversky term of the training loss (drs_patch_dice_coeffs, drs_classifier_loss_dice,
drs_net_set_dice) costs, in one process on one device, at the headline step's shape (128 patches of 64 x 64, K = 6): HIP-event times of
  - the classifier's inference form into the logits (the pre-pass's first launch), drs_patch_dice_coeffs over them, and the fused
    classifier (C = 256: the LDS-DMA form, training) without coefficients (drs_classifier_loss_pixel) and with them
    (drs_classifier_loss_dice), plain and with gamma = 2,
each launched `warmup` times untimed, then `reps` times, one event pair per launch, the arms interleaved so that a drift of the clocks
meets all of them; the median and the extremes are reported.  Then the whole training step of the headline net (dilated_grsl_rate8,
5 bands) with the option off and on (lam = 1, alpha = beta = 0.5, smooth = 1), alternately, by event pairs around `steps` steps each:
the share of the step the option costs; and the engine's own timing kind "classifier_loss" per step, off and on.  Prints one JSON line
and writes it to out=.

    python tools/bench_dice_loss.py [B=128] [S=64] [reps=15] [warmup=3] [steps=10] [rounds=5] [out=profiles/dice_loss/cost.json]"""
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
DICE = (1.0, 0.5, 0.5, 1.0)
OPTIONS = ("B", "S", "reps", "warmup", "steps", "rounds", "out")


def main(B, S, reps, warmup, steps, rounds, out_path):
    assert torch.cuda.is_available(), "bench_dice_loss.py measures on the device: there is no CPU path"
    _lib.load()
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

    def infer():
        _lib.call("drs_classifier_loss_pixel", feat.data_ptr(), B, S, 0, C, 0, C, K, w.data_ptr(), b.data_ptr(), None, None, None, 1.0, None, 0.0,
                  None, logits.data_ptr(), None, None, 0, 0, None, None, None, None, st)

    def coeffs():
        _lib.call("drs_patch_dice_coeffs", logits.data_ptr(), lab.data_ptr(), None, B, S, K, *DICE, None, coef.data_ptr(), ploss.data_ptr(), st)

    def cls(gamma, with_coef):
        head = (feat.data_ptr(), B, S, 0, C, 0, C, K, w.data_ptr(), b.data_ptr(), lab.data_ptr(), None, valid.data_ptr(), 1.0 / M, None, gamma, None)
        tail = (None, pred.data_ptr(), gfeat.data_ptr(), C, 0, dwp.data_ptr(), dbp.data_ptr(), lp.data_ptr(), conf.data_ptr(), st)
        if not with_coef:
            return lambda: _lib.call("drs_classifier_loss_pixel", *(head + tail))
        return lambda: _lib.call("drs_classifier_loss_dice", *(head + (coef.data_ptr(),) + tail))
    infer()
    coeffs()
    torch.cuda.synchronize()
    arms = {"classifier_inference_logits": infer, "dice_coeffs": coeffs, "classifier_plain": cls(0.0, False), "classifier_plain_dice": cls(0.0, True),
            "classifier_focal": cls(2.0, False), "classifier_focal_dice": cls(2.0, True)}
    res = {"workload": "%d patches of %d x %d, K = %d; classifier C = %d, training" % (B, S, S, K, C), "reps": reps, "warmup": warmup,
           "dice": list(DICE)}
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
        for name, dice in (("off", None), ("on", DICE)):
            net.set_dice(dice)
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
    res["kernels_share_of_step"] = round((res["classifier_inference_logits_ms"]["median"] + res["dice_coeffs_ms"]["median"]
                                          + res["classifier_plain_dice_ms"]["median"] - res["classifier_plain_ms"]["median"]) / off, 5)
    # the engine's own timing kind of the classifier bracket (the pre-pass is accounted there), per step
    for name, dice in (("off", None), ("on", DICE)):
        net.set_dice(dice)
        net.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        net.timer = True
        for _ in range(steps):
            net.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        kind = net.timer.summary()["classifier_loss"]
        net.timer = None
        res["engine_classifier_loss_kind_%s_ms_per_step" % name] = round(kind["ms"] / steps, 4)
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
        sys.exit("bench_dice_loss.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("B", 128)), int(kw.get("S", 64)), int(kw.get("reps", 15)), int(kw.get("warmup", 3)), int(kw.get("steps", 10)),
         int(kw.get("rounds", 5)), kw.get("out", os.path.join(ROOT, "profiles", "dice_loss", "cost.json")))
