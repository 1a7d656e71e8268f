#!/usr/bin/env python3
"""BASELINE config 5's workload in both inference modes, in one process: the reference's sliding windows (loops.predict_tile, 64 x 64
windows at stride 32, batches of 256) and overlap-tile inference (loops.predict_tile_dense, tiles of 512).  The mosaic, its statistics
and the net's moving statistics are built exactly as bench.py's baseline_configs builds config 5 (6000 x 6000 x 5 on the device,
Dilated8Pooling, moving statistics from one train-mode pass over 256 spread windows).  Every shape is warmed up first; each mode then
runs `reps` times, alternating, timed by a host clock around a device synchronize.  Prints one JSON line.
tta=flip|d4 adds a third mode: overlap-tile inference with that dihedral test-time augmentation (predict_tile_dense(..., tta=...)),
on its own symmetric-margin plan.  scales=0.75,1,1.25 adds the multi-scale test-time augmentation mode (predict_tile_dense(...,
scales=...); with tta= as well, both at once), every scale's tile shapes warmed up too.
se=global is a mode of its own: the squeeze-and-excitation net (dilated_icpr_rate6_SE), its sliding-window map at S = 64 against its
overlap-tile map with whole-image gates (predict_tile_dense(..., se="global")) -- the plain dense mode does not exist
for that net.
    python tools/bench_dense_predict.py [mosaic=6000] [tile=512] [reps=3] [tta=flip|d4] [scales=0.75,1,1.25] [se=global]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drs_amd.net import DilatedNet  # noqa: E402
from drs_amd import _lib, loops, patches as P  # noqa: E402

NET, CH, K, WD = "dilated_grsl_rate8", 5, 6, 0.005
PEAK_FP32_MFMA_TFLOPS = 157.3     # MI355X fp32 MFMA rate (bench.py's figure)


def checksum(pred):
    idx = torch.arange(pred.numel(), device=pred.device, dtype=torch.int64)
    return int(((pred.reshape(-1).long() + 1) * (idx % 65521 + 1)).sum().item() % (1 << 61))


def setup(net_type, mosaic):
    """config 5's mosaic on the device, its statistics, and `net_type` with moving statistics from one train-mode pass over 256 spread
    windows"""
    dev = "cuda:0"
    n, S, Bw = int(mosaic), 64, 256
    g0 = torch.Generator(device=dev).manual_seed(5)
    m = torch.rand(5, n, n, device=dev, generator=g0)
    m[:3] = torch.nn.functional.avg_pool2d(m[:3].unsqueeze(0), 9, stride=1, padding=4, count_include_pad=False)[0]
    m[4] *= 0.2
    mosaic_t = m.permute(1, 2, 0).contiguous().reshape(-1)
    mean = m[:3].mean(dim=(1, 2)).tolist()
    std = m[:3].std(dim=(1, 2)).tolist()
    del m
    pool = P.TilePool([np.zeros((S, S, CH), dtype=np.float32)], None, dev, dtype=np.float32)      # shell; the mosaic is on the device
    pool.tiles, pool.labels = mosaic_t, torch.zeros(n * n, dtype=torch.uint8, device=dev)
    pool.h, pool.w = [n], [n]
    pool.tile_h = torch.tensor([n], dtype=torch.int32, device=dev)
    pool.tile_w = torch.tensor([n], dtype=torch.int32, device=dev)
    net = DilatedNet(net_type, CH, K, WD, b_max=Bw, s_max=S, device=dev, seed=42)
    nh, nw = P.window_counts(n, n, S, S // 2)
    spread = np.linspace(0, nh * nw - 1, Bw).astype(np.int64)
    allpos = np.stack([np.minimum((spread // nw) * (S // 2), n - S), np.minimum((spread % nw) * (S // 2), n - S)], axis=1)
    P.crop_to_net(net, pool, np.concatenate([np.zeros((Bw, 1), dtype=np.int64), allpos], axis=1), S, mean, std)
    net.train_step(Bw, S, 0.0, apply_update=False)
    torch.cuda.synchronize()
    for i, L in enumerate(net.plan.layers):
        mr = net.mean_rstd[i].cpu().numpy().reshape(L.cout, 2).astype(np.float64)
        net.set_variable(L.name + "/moving_mean", mr[:, 0])
        net.set_variable(L.name + "/moving_variance", np.maximum(1.0 / mr[:, 1] ** 2 - 1e-3, 1e-6))
    return dev, n, S, Bw, pool, net, mean, std, nh, nw, allpos


def main_se(mosaic=6000, tile=512, reps=3):
    """se=global: the SE net's window map against its overlap-tile map with whole-image gates"""
    net_type = "dilated_icpr_rate6_SE"
    dev, n, S, Bw, pool, net, mean, std, nh, nw, allpos = setup(net_type, mosaic)
    # (the initialiser's fully connected SE weights, stddev 0.005, leave every gate at sigmoid(0.1): give the gates something to do)
    g1 = torch.Generator(device="cpu").manual_seed(7)
    for name in net.variable_names():
        if "_fc" in name and name.endswith("/weights"):
            net.set_variable(name, (torch.randn(net.get_variable(name).shape, generator=g1) * 0.3).numpy())
    T = min(n, int(tile))
    before, after = net.plan.gated_receptive_field
    boxes = P.dense_tiles(n, n, T, before, after)
    B_t = loops.dense_batch(net.plan, T)
    for b in sorted({Bw, nh * nw % Bw} - {0}):
        P.crop_to_net(net, pool, np.concatenate([np.zeros((b, 1), dtype=np.int64), allpos[:b]], axis=1), S, mean, std)
        net.forward(b, S)
    twin = loops.dense_twin(net, T, B_t)
    n_se = len(net.plan.se)
    boxes_dev = torch.from_numpy(boxes.astype(np.int32)).to(dev)
    for b in sorted({B_t, len(boxes) % B_t} - {0}):          # every shape of every sweep, code objects loaded outside the timing
        P.crop_to_net(twin, pool, np.concatenate([np.zeros((b, 1), dtype=np.int64), boxes[:b, :2]], axis=1), T, mean, std)
        for j in range(n_se):
            twin.forward_staged(b, T, j, boxes_dev.data_ptr())
            twin.se_gate_finish(j, float(n) * n)
        twin.forward_staged(b, T, n_se)
    torch.cuda.synchronize()
    modes = ("window", "dense_se")
    runs, maps = {m: [] for m in modes}, {}
    for _ in range(int(reps)):
        for mode in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "window":
                pred, _ = loops.predict_tile(net, pool, 0, S, Bw, mean, std)
            else:
                pred, _ = loops.predict_tile_dense(net, pool, 0, B_t, mean, std, tile=T, se="global")
            torch.cuda.synchronize()
            runs[mode].append(time.perf_counter() - t0)
            maps[mode] = pred
    # MACs per pixel of a sweep: the blocks up to the one SE j follows; the last sweep is the whole net
    per_block = [L.k * L.k * L.cin * L.cout for L in net.plan.layers]
    sweeps = [sum(per_block[:li + 1]) for li in sorted(net.plan.se)] + [net.plan.mac_per_pixel()]
    mac = {"window": net.plan.mac_per_pixel() * nh * nw * S * S, "dense_se": sum(sweeps) * len(boxes) * T * T}
    out = dict(workload="BASELINE config 5's mosaic (%dx%dx5) with %s on ONE GPU: sliding windows 64x64 at stride 32 in batches of 256 "
                        "(every window gated by its own mean) vs overlap-tile inference with whole-image gates at T = %d (%d sweeps "
                        "over %d tiles, %d tiles per forward)" % (n, n, net_type, T, n_se + 1, len(boxes), B_t),
               gated_receptive_field=[before, after], tiles=len(boxes), windows=nh * nw, reps=int(reps),
               sweep_mac_per_pixel=sweeps, sweeps_vs_one_pass=round(sum(sweeps) / sweeps[-1], 3))
    for mode in modes:
        best = min(runs[mode])
        flops = 2.0 * mac[mode]
        out[mode] = dict(seconds=[round(v, 3) for v in runs[mode]], best_s=round(best, 3), map_mpx_per_s=round(n * n / best / 1e6, 2),
                         flop=flops, fp32_floor_s=round(flops / (PEAK_FP32_MFMA_TFLOPS * 1e12), 3),
                         fp32_ceiling_frac=round(flops / best / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4))
    out["dense_se_vs_window_time"] = round(out["dense_se"]["best_s"] / out["window"]["best_s"], 3)
    out["dense_se_vs_window_flop_predicted"] = round(mac["dense_se"] / mac["window"], 3)
    out["maps_agree_frac"] = round(float((maps["window"] == maps["dense_se"]).float().mean().item()), 5)     # for information only
    out["dense_se_map_checksum"] = "sum((label+1) * (flat_index %% 65521 + 1)) mod 2^61 = %d" % checksum(maps["dense_se"])
    out["window_map_checksum"] = "sum((label+1) * (flat_index %% 65521 + 1)) mod 2^61 = %d" % checksum(maps["window"])
    print(json.dumps(out))


def main(mosaic=6000, tile=512, reps=3, tta=None, scales=None, se=None):
    if se is not None:
        if se != "global" or tta is not None or scales is not None:
            sys.exit("se=global is a mode of its own (no tta= / scales= beside it)")
        return main_se(mosaic, tile, reps)
    dev, n, S, Bw, pool, net, mean, std, nh, nw, allpos = setup(NET, mosaic)

    T = min(n, int(tile))
    before, after = net.plan.receptive_field
    boxes = P.dense_tiles(n, n, T, before, after)
    B_t = loops.dense_batch(net.plan, T)
    # warm-up: every shape each mode launches (full and last partial batch), code objects loaded outside the timing
    rest_w = nh * nw % Bw
    for b in sorted({Bw, rest_w} - {0}):
        P.crop_to_net(net, pool, np.concatenate([np.zeros((b, 1), dtype=np.int64), allpos[:b]], axis=1), S, mean, std)
        net.forward(b, S)
    twin = loops.dense_twin(net, T, B_t)
    for b in sorted({B_t, len(boxes) % B_t} - {0}):
        P.crop_to_net(twin, pool, np.concatenate([np.zeros((b, 1), dtype=np.int64), boxes[:b, :2]], axis=1), T, mean, std)
        twin.forward(b, T)
    modes = ("window", "dense")
    if tta is not None:
        G = P.tta_group(tta)
        m = max(before, after)
        boxes_tta = P.dense_tiles(n, n, T, m, m)
        for b in sorted({B_t, len(boxes_tta) % B_t} - {0}):
            for g in G:
                P.crop_dihedral_to_net(twin, pool, np.concatenate([np.zeros((b, 1), dtype=np.int64), boxes_tta[:b, :2]], axis=1), T,
                                       mean, std, g)
                twin.forward(b, T)
        modes = modes + ("dense_tta",)
    if scales is not None:
        scales = P.check_scales([float(v) for v in str(scales).split(",")])
        Gs = (0,) if tta is None else P.tta_group(tta)
        ms = (max(before, after),) * 2 if any(Gs) else (before, after)
        plans = []
        for s in scales:
            ns = P.scaled_size(n, s)
            Ts = min(ns, T)
            plans.append((s, ns, Ts, P.dense_tiles(ns, ns, Ts, *ms)))
            for b in sorted({B_t, len(plans[-1][3]) % B_t} - {0}):
                for g in Gs:
                    P.crop_resampled_to_net(twin, pool, np.concatenate([np.zeros((b, 1), dtype=np.int64), plans[-1][3][:b, :2]], axis=1),
                                            Ts, ns, ns, mean, std, g)
                    twin.forward(b, Ts)
        one = torch.ones(K, dtype=torch.float32, device=dev)
        occ1 = torch.ones(1, dtype=torch.int32, device=dev)
        for is_prob in (0, 1):
            _lib.call("drs_resample_accumulate", one.data_ptr(), occ1.data_ptr(), 1, 1, K, is_prob, 1, 1, one.data_ptr(), twin._stream())
        modes = modes + ("dense_scales",)
    torch.cuda.synchronize()

    runs = {mode: [] for mode in modes}
    maps = {}
    for _ in range(int(reps)):
        for mode in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if mode == "window":
                pred, _ = loops.predict_tile(net, pool, 0, S, Bw, mean, std)
            elif mode == "dense":
                pred, _ = loops.predict_tile_dense(net, pool, 0, B_t, mean, std, tile=T)
            elif mode == "dense_tta":
                pred, _ = loops.predict_tile_dense(net, pool, 0, B_t, mean, std, tile=T, tta=tta)
            else:
                pred, _ = loops.predict_tile_dense(net, pool, 0, B_t, mean, std, tile=T, tta=tta, scales=scales)
            torch.cuda.synchronize()
            runs[mode].append(time.perf_counter() - t0)
            maps[mode] = pred
    mac = net.plan.mac_per_pixel()
    pix = {"window": nh * nw * S * S, "dense": len(boxes) * T * T}
    if tta is not None:
        pix["dense_tta"] = len(G) * len(boxes_tta) * T * T
    if scales is not None:
        pix["dense_scales"] = len(Gs) * sum(len(bx) * Ts * Ts for _, _, Ts, bx in plans)
    out = dict(workload="BASELINE config 5: dilated_grsl_rate8 inference of a %dx%dx5 synthetic mosaic on ONE GPU; sliding windows "
                        "64x64 at stride 32 in batches of 256 (overlap-add, the reference's map) vs overlap-tile inference at T = %d "
                        "(exact whole-tile forward, %d tiles per forward)" % (n, n, T, B_t),
               receptive_field=[before, after], tiles=len(boxes), windows=nh * nw, reps=int(reps))
    for mode in modes:
        best = min(runs[mode])
        flops = 2.0 * mac * pix[mode]
        out[mode] = dict(seconds=[round(v, 3) for v in runs[mode]], best_s=round(best, 3), map_mpx_per_s=round(n * n / best / 1e6, 2),
                         pixel_forwards=pix[mode], flop=flops, fp32_floor_s=round(flops / (PEAK_FP32_MFMA_TFLOPS * 1e12), 3),
                         fp32_ceiling_frac=round(flops / best / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4))
    out["speedup_best"] = round(out["window"]["best_s"] / out["dense"]["best_s"], 3)
    out["pixel_forward_ratio"] = round(pix["window"] / pix["dense"], 3)
    out["maps_agree_frac"] = round(float((maps["window"] == maps["dense"]).float().mean().item()), 5)     # for information only
    if tta is not None:
        out["tta"] = dict(group=tta, codes=list(G), tiles=len(boxes_tta), symmetric_margin=m,
                          cost_vs_dense=round(out["dense_tta"]["best_s"] / out["dense"]["best_s"], 3),
                          maps_agree_with_dense_frac=round(float((maps["dense_tta"] == maps["dense"]).float().mean().item()), 5),
                          map_checksum="sum((label+1) * (flat_index %% 65521 + 1)) mod 2^61 = %d" % checksum(maps["dense_tta"]))
    if scales is not None:
        tiles_one = len(P.dense_tiles(n, n, T, *ms))
        out["scales"] = dict(factors=list(scales), tta=tta, sides=[ns for _, ns, _, _ in plans], tile_sides=[Ts for _, _, Ts, _ in plans],
                             tiles=[len(bx) for _, _, _, bx in plans],
                             predicted_cost_vs_one_scale=round(sum(len(bx) for _, _, _, bx in plans) / tiles_one, 3),
                             cost_vs_dense=round(out["dense_scales"]["best_s"] / out["dense"]["best_s"], 3),
                             maps_agree_with_dense_frac=round(float((maps["dense_scales"] == maps["dense"]).float().mean().item()), 5),
                             map_checksum="sum((label+1) * (flat_index %% 65521 + 1)) mod 2^61 = %d" % checksum(maps["dense_scales"]))
    out["dense_map_checksum"] = "sum((label+1) * (flat_index %% 65521 + 1)) mod 2^61 = %d" % checksum(maps["dense"])
    out["window_map_checksum"] = "sum((label+1) * (flat_index %% 65521 + 1)) mod 2^61 = %d" % checksum(maps["window"])
    print(json.dumps(out))


if __name__ == "__main__":
    main(**{k: (v if k in ("tta", "scales", "se") else int(v)) for k, v in (a.split("=", 1) for a in sys.argv[1:])})
