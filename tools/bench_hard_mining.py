#!/usr/bin/env python3
"""What online hard example mining in the training loss (drs_patch_hard_weight, drs_net_set_hard_mining) costs, in one
process on one device: HIP-event times of
  - the classifier's inference form into the logits (the pre-pass's first launch; C = 256, K = 6) and drs_patch_hard_weight over
    them at the headline step's shape (128 patches of 64 x 64), at keep = 0.25 and 1/4096, on the logits of random features (distinct
    keys) and on logits so confident that every key is +0 (one tie over the whole patch: the worst case of the LDS histogram and of the
    tie pass), with and without an incoming map; and the weight kernel alone at one rank's shape of an 8-rank run (16 x 85 x 85),
each launched `warmup` times untimed, then `reps` times, one event pair per launch, the arms interleaved so that a drift of the clocks
meets all of them; the median and the extremes are reported.  Then the whole training step of the headline net (dilated_grsl_rate8,
5 bands) with the option off and on (keep = 0.25), alternately, by event pairs around `steps` steps each: the share of the step the
option costs; and the engine's own timing kind "classifier_loss" per step, off and on.  Prints one JSON line and writes it to out=.

    python tools/bench_hard_mining.py [B=128] [S=64] [reps=15] [warmup=3] [steps=10] [rounds=5] [out=profiles/hard_mining/cost.json]"""
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
HM = (0.25, 0)
RANK_SHAPE = (16, 85)
OPTIONS = ("B", "S", "reps", "warmup", "steps", "rounds", "out")


def main(B, S, reps, warmup, steps, rounds, out_path):
    assert torch.cuda.is_available(), "bench_hard_mining.py measures on the device: there is no CPU path"
    _lib.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    M = B * S * S
    lab, valid = blob_labels(B, S)
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    feat = torch.randn(M * C, device=DEV, generator=g)
    w = torch.randn(C * K, device=DEV, generator=g) / 16
    b = torch.zeros(K, device=DEV)
    logits = torch.empty(M * K, device=DEV)
    sure = torch.zeros(M, K, device=DEV)
    sure[torch.arange(M, device=DEV), lab.reshape(-1).long()] = 60.0          # every key exactly +0
    sure = sure.reshape(-1).contiguous()
    ce, weight = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    w_in = 1.0 + 10.0 * torch.rand(M, device=DEV, generator=g)
    Br, Sr = RANK_SHAPE
    Mr = Br * Sr * Sr
    lab_r, _ = blob_labels(Br, Sr)
    logits_r = torch.randn(Mr * K, device=DEV, generator=g) * 2.0
    ce_r, weight_r = torch.empty(Mr, device=DEV), torch.empty(Mr, device=DEV)

    def infer():
        _lib.call("drs_classifier_loss_pixel", feat.data_ptr(), B, S, 0, C, 0, C, K, w.data_ptr(), b.data_ptr(), None, None, None, 1.0, None, 0.0,
                  None, logits.data_ptr(), None, None, 0, 0, None, None, None, None, st)

    def hard(lg, keep, pw=None):
        return lambda: _lib.call("drs_patch_hard_weight", lg.data_ptr(), ce.data_ptr(), lab.data_ptr(), None, B, S, K, keep, 0,
                                 None if pw is None else pw.data_ptr(), weight.data_ptr(), None, st)

    def hard_rank():
        _lib.call("drs_patch_hard_weight", logits_r.data_ptr(), ce_r.data_ptr(), lab_r.data_ptr(), None, Br, Sr, K, HM[0], 0, None,
                  weight_r.data_ptr(), None, st)
    infer()
    torch.cuda.synchronize()
    arms = {"classifier_inference_logits": infer, "hard_weight_keep_0.25": hard(logits, 0.25), "hard_weight_keep_1_4096": hard(logits, 1.0 / 4096),
            "hard_weight_keep_0.25_with_map": hard(logits, 0.25, w_in), "hard_weight_keep_0.25_all_keys_zero": hard(sure, 0.25),
            "hard_weight_%dx%dx%d_keep_0.25" % (Br, Sr, Sr): hard_rank}
    res = {"workload": "%d patches of %d x %d, K = %d; classifier C = %d; one rank's shape %d x %d x %d" % (B, S, S, K, C, Br, Sr, Sr),
           "reps": reps, "warmup": warmup, "hard_mining": list(HM)}
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
        for name, hm in (("off", None), ("on", HM)):
            net.set_hard_mining(hm)
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
    res["kernels_share_of_step"] = round((res["classifier_inference_logits_ms"]["median"] + res["hard_weight_keep_0.25_ms"]["median"]) / off, 5)
    # the engine's own timing kind of the classifier bracket (the pre-pass is accounted there), per step
    for name, hm in (("off", None), ("on", HM)):
        net.set_hard_mining(hm)
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
        sys.exit("bench_hard_mining.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("B", 128)), int(kw.get("S", 64)), int(kw.get("reps", 15)), int(kw.get("warmup", 3)), int(kw.get("steps", 10)),
         int(kw.get("rounds", 5)), kw.get("out", os.path.join(ROOT, "profiles", "hard_mining", "cost.json")))
