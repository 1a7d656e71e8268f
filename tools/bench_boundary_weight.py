#!/usr/bin/env python3
"""What the boundary-weighted loss (drs_patch_boundary_weight, drs_classifier_loss_pixel) costs, in one process on one
device, at the headline step's shape (128 patches of 64 x 64, K = 6): HIP-event times of
  - drs_patch_boundary_weight on blob labels with a rotated-corner validity map, at R = 4, 12 and 16 (sigma = R / 3), and on uniform
    patches at R = 16 (no pixel leaves its scan early: the worst case of the ring scan),
  - the fused classifier (C = 256: the LDS-DMA form, training) without a map (drs_classifier_loss_focal) and with one
    (drs_classifier_loss_pixel), plain and with gamma = 2,
each launched `warmup` times untimed, then `reps` times, one event pair per launch, the arms interleaved so that a drift of the clocks
meets all of them; the median and the extremes are reported.  Then the whole training step of the headline net (dilated_grsl_rate8,
5 bands) with the option off and on (a = 10, sigma = 4, R = 12), alternately, by event pairs around `steps` steps each: the share of
the step the option costs.  Prints one JSON line and writes it to out=.

    python tools/bench_boundary_weight.py [B=128] [S=64] [reps=15] [warmup=3] [steps=10] [rounds=5] [out=profiles/boundary_weight/bench.json]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drs_amd import _lib  # noqa: E402

DEV = "cuda:0"
K, C, CH, NET = 6, 256, 5, "dilated_grsl_rate8"
OPTIONS = ("B", "S", "reps", "warmup", "steps", "rounds", "out")


def blob_labels(B, S, seed=0, seeds=8):
    """uint8 [B][S][S] on the device: per patch the nearest of `seeds` random points, classes 0..K-1; and a validity map whose
    corners are cut as a rotation by 30 degrees cuts them (labels 0 there, as the crop kernel fills them)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pts = (torch.rand((B, seeds, 2), generator=g) * S).to(DEV)
    cls = torch.randint(0, K, (B, seeds), generator=g).to(DEV)
    ys = torch.arange(S, device=DEV, dtype=torch.float32)
    d = (ys[None, :, None, None] - pts[:, None, None, :, 0]) ** 2 + (ys[None, None, :, None] - pts[:, None, None, :, 1]) ** 2
    lab = torch.gather(cls, 1, d.argmin(dim=-1).reshape(B, -1)).reshape(B, S, S).to(torch.uint8)
    c = (S - 1) / 2.0
    u = (ys[None, :] - c) * np.cos(np.pi / 6) + (ys[:, None] - c) * np.sin(np.pi / 6)
    v = -(ys[None, :] - c) * np.sin(np.pi / 6) + (ys[:, None] - c) * np.cos(np.pi / 6)
    valid = ((u.abs() <= 0.42 * S + 0.5) & (v.abs() <= 0.42 * S + 0.5)).to(torch.uint8)[None].repeat(B, 1, 1)
    lab = lab * valid
    return lab.contiguous(), valid.contiguous()


def timed(arms, reps, warmup):
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
    return {name + "_ms": {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)} for name, t in times.items()}


def main(B, S, reps, warmup, steps, rounds, out_path):
    assert torch.cuda.is_available(), "bench_boundary_weight.py measures on the device: there is no CPU path"
    _lib.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    M = B * S * S
    lab, valid = blob_labels(B, S)
    uniform = torch.full((B, S, S), 3, dtype=torch.uint8, device=DEV)
    weight = torch.empty(M, dtype=torch.float32, device=DEV)
    d2 = torch.empty(M, dtype=torch.int16, device=DEV)

    def wk(labels, val, R):
        sigma = R / 3.0
        return lambda: _lib.call("drs_patch_boundary_weight", labels.data_ptr(), None if val is None else val.data_ptr(), B, S, R, 10.0,
                                 1.0 / (2.0 * sigma * sigma), None, weight.data_ptr(), st)
    arms = {"weight_R4": wk(lab, valid, 4), "weight_R12": wk(lab, valid, 12), "weight_R16": wk(lab, valid, 16),
            "weight_R16_uniform": wk(uniform, None, 16),
            "weight_R12_with_d2": lambda: _lib.call("drs_patch_boundary_weight", lab.data_ptr(), valid.data_ptr(), B, S, 12, 10.0, 1.0 / 32.0,
                                                    d2.data_ptr(), weight.data_ptr(), st)}
    # the classifier at the same shape
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    feat = torch.randn(M * C, device=DEV, generator=g)
    w = torch.randn(C * K, device=DEV, generator=g) / 16
    b = torch.zeros(K, device=DEV)
    rows = _lib.query("drs_classifier_rows", B, S)
    gfeat = torch.empty(M * C, device=DEV)
    pred = torch.empty(M, dtype=torch.uint8, device=DEV)
    dwp, dbp = torch.empty(rows * C * K, device=DEV), torch.empty(rows * K, device=DEV)
    lp = torch.empty(rows, dtype=torch.float64, device=DEV)
    conf = torch.zeros(K * K, dtype=torch.int32, device=DEV)
    wk(lab, valid, 12)()
    torch.cuda.synchronize()
    pw = weight.clone()

    def cls(gamma, pmap):
        head = (feat.data_ptr(), B, S, 0, C, 0, C, K, w.data_ptr(), b.data_ptr(), lab.data_ptr(), None, valid.data_ptr(), 1.0 / M, None, gamma)
        tail = (None, pred.data_ptr(), gfeat.data_ptr(), C, 0, dwp.data_ptr(), dbp.data_ptr(), lp.data_ptr(), conf.data_ptr(), st)
        if pmap is None:
            return lambda: _lib.call("drs_classifier_loss_focal", *(head + tail))
        return lambda: _lib.call("drs_classifier_loss_pixel", *(head + (pmap.data_ptr(),) + tail))
    arms.update({"classifier_plain": cls(0.0, None), "classifier_plain_map": cls(0.0, pw), "classifier_focal": cls(2.0, None),
                 "classifier_focal_map": cls(2.0, pw)})
    res = {"workload": "%d patches of %d x %d, K = %d; classifier C = %d, training" % (B, S, S, K, C), "reps": reps, "warmup": warmup}
    res.update(timed(arms, reps, warmup))
    res["finite_distance_share_R12"] = round(float((pw != 1.0).float().mean().item()), 4)
    del feat, gfeat
    # the whole step, option off and on, alternately
    from drs_amd.net import DilatedNet
    net = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=42)
    rng = np.random.default_rng(0)
    x = rng.normal(size=(B, S * S * CH)).astype(np.float32)
    net.feed(x, lab.cpu().numpy().reshape(B, -1), S, acc_mask=valid.cpu().numpy().reshape(B, -1))
    step_ms = {"off": [], "on": []}
    for r in range(rounds + 1):
        for name, bw in (("off", None), ("on", (10.0, 4.0, 12))):
            net.set_boundary_weight(bw)
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
    res["kernels_share_of_step"] = round((res["weight_R12_ms"]["median"] + res["classifier_plain_map_ms"]["median"]
                                          - res["classifier_plain_ms"]["median"]) / off, 5)
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
        sys.exit("bench_boundary_weight.py: unknown argument %s; expected %s" % (bad[0], " ".join("[%s=...]" % o for o in OPTIONS)))
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("B", 128)), int(kw.get("S", 64)), int(kw.get("reps", 15)), int(kw.get("warmup", 3)), int(kw.get("steps", 10)),
         int(kw.get("rounds", 5)), kw.get("out", os.path.join(ROOT, "profiles", "boundary_weight", "bench.json")))
