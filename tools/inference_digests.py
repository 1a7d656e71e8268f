#!/usr/bin/env python3
"""SHA-256 digests of everything the whole-map inference paths of loops.py return, print and write, for fixed seeds: the yardstick of a
change that must leave them bit for bit (run it on the tree before and on the tree after, on the same machine, and compare the two
JSON objects).  Only public functions are called -- predict_tile, predict_tile_multiscale, predict_tile_dense, validate_test,
generate_final_maps, fit_temperature -- so the same file runs on either tree.

Cases (every predict_* case in three forms: return_sums; scores = confidence, margin, entropy; those scores at temperature_beta 0.5):
  window        dilated_grsl, 5 bands, K = 6, a 70 x 62 map, windows of 25
  window_k2     the same with K = 2 (the smallest instantiation of the score kernels that has a margin)
  multisize     windows of 25 and 33
  dense/*       dilated_grsl, K = 6, a 160 x 150 map, tile 80 (8 x 7 ragged tiles; 5 tile rows at scale 0.75): plain, tta flip, tta d4,
                scales (0.75, 1.25), scales with flip
  dense_se/*    dilated_icpr_rate6_SE, se="global", a 96 x 88 map, tile 64: plain, d4, scales (0.75, 1.25).  (Its margins are 27 + 28,
                28 + 28 with d4, so a tile side must exceed 56.)
  validate_test / generate_final_maps / fit_temperature over two labelled maps on the windows, the multi-size windows, dense d4 and dense
                scales: printed lines, confusion matrix, maps, `extra`, the files written (name and bytes), beta's float32 bits
  two_ranks/*   two processes on the one GPU (gloo), as the two-rank tests run them: the window bands, the round-robin windows
                (return_sums), the multi-size windows, dense plain / d4 / scales + flip, the SE net, and validate_test on dense d4
    python tools/inference_digests.py [out=FILE] [ranks=1|2]
"""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
CH = 5
KINDS = ("confidence", "margin", "entropy")
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
SE_NET = "dilated_icpr_rate6_SE"


def sha(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        return hashlib.sha256(str((x.dtype.str, x.shape)).encode() + x.tobytes()).hexdigest()
    if isinstance(x, bytes):
        return hashlib.sha256(x).hexdigest()
    return hashlib.sha256(repr(x).encode()).hexdigest()


def make_net(net_type, K, b_max, s_max, seed=3, comm=None):
    """random moving statistics, the classifier kernel scaled so that the score maps span the byte range, SE gates given something to do"""
    from drs_amd.net import DilatedNet
    rng = np.random.default_rng(seed)
    d = DilatedNet(net_type, CH, K, 0.005, b_max=b_max, s_max=s_max, device=DEV, seed=seed, **({} if comm is None else {"comm": comm}))
    for n in d.variable_names():
        v = d.get_variable(n)
        if n.endswith("moving_mean"):
            d.set_variable(n, (rng.normal(size=v.shape) * 0.1).astype(np.float32))
        elif n.endswith("moving_variance"):
            d.set_variable(n, rng.uniform(0.5, 2.0, size=v.shape).astype(np.float32))
        elif "_fc" in n and n.endswith("/weights"):
            d.set_variable(n, (rng.normal(size=v.shape) * 0.3).astype(np.float32))
    d.set_variable("conv_classifier/weights", d.get_variable("conv_classifier/weights") * np.float32(16.0))
    return d


def make_tile(h, w, K, seed):
    from drs_amd.synthetic import make_tile as mk
    return mk(h, w, CH, K, seed=seed, n_seeds=30)


def three_forms(out, name, fn, count=True):
    """fn(**kw) is one public predict_* call; its three forms into out[name/...]"""
    res = fn(return_sums=True)
    out[name + "/sums"], out[name + "/occur"] = sha(res[0]), sha(res[1])
    if count:
        out[name + "/count"] = int(res[2])
    for form, kw in (("scores", dict(scores=KINDS)), ("beta", dict(scores=KINDS, temperature_beta=0.5))):
        res = fn(**kw)
        out["%s/%s/labels" % (name, form)] = sha(res[0])
        for k, v in res[-1].items():
            out["%s/%s/%s" % (name, form, k)] = sha(v)
    out[name + "/labels"] = sha(fn()[0] if count else fn())


def dense_cases(net_type):
    if net_type == SE_NET:
        return (("plain", dict()), ("d4", dict(tta="d4")), ("scales", dict(scales=(0.75, 1.25))))
    return (("plain", dict()), ("flip", dict(tta="flip")), ("d4", dict(tta="d4")), ("scales", dict(scales=(0.75, 1.25))),
            ("scales_flip", dict(scales=(0.75, 1.25), tta="flip")))


def predict_cases(out, comm=None, pre=""):
    from drs_amd import loops, patches as P
    ckw = {} if comm is None else {"comm": comm}
    for name, K in (("window", 6), ("window_k2", 2)):
        d = make_net("dilated_grsl", K, 5, 33, seed=4, comm=comm)
        pool = P.TilePool([make_tile(70, 62, K, seed=12)[0]], None, DEV)
        three_forms(out, pre + name, lambda **kw: loops.predict_tile(d, pool, 0, 25, 5, MEAN, STD, **ckw, **kw))
        if K == 6:
            three_forms(out, pre + "multisize", lambda **kw: loops.predict_tile_multiscale(d, pool, 0, [25, 33], 5, MEAN, STD, **ckw, **kw),
                        count=False)
    for net_type, (h, w), tile, tag in (("dilated_grsl", (160, 150), 80, "dense"), (SE_NET, (96, 88), 64, "dense_se")):
        d = make_net(net_type, 6, 2, 24, seed=3)
        pool = P.TilePool([make_tile(h, w, 6, seed=11)[0]], None, DEV)
        se = dict(se="global") if net_type == SE_NET else {}
        for name, kw0 in dense_cases(net_type):
            if comm is not None and name in ("flip", "scales"):
                continue
            three_forms(out, "%s%s/%s" % (pre, tag, name),
                        lambda **kw: loops.predict_tile_dense(d, pool, 0, 4, MEAN, STD, tile=tile, **ckw, **se, **kw0, **kw))


def loop_cases(out, comm=None, pre="", paths=None):
    """validate_test, generate_final_maps and fit_temperature over two labelled maps"""
    from drs_amd import loops
    rank0 = comm is None or comm.rank == 0
    ckw = {} if comm is None else {"comm": comm}
    all_paths = {"windows": ((44, 50), dict()), "multisize": ((44, 50), dict(crop_sizes=[25, 18])),
                 "dense_d4": ((160, 150), dict(dense_tile=96, dense_tta="d4")),
                 "dense_scales": ((160, 150), dict(dense_tile=96, dense_scales=(0.75, 1.25)))}
    d = make_net("dilated_grsl", 6, 6, 25, seed=5, comm=comm)
    for name in paths or all_paths:
        (h, w), kw = all_paths[name]
        tiles = [make_tile(h, w, 6, seed=21), make_tile(h, w, 6, seed=22)]
        data = [t[0] for t in tiles]
        rng = np.random.default_rng(2)
        labs = [np.where(rng.uniform(size=(h, w)) < 0.1, 6, t[1]).astype(np.uint8) for t in tiles]      # 6 = eroded boundary, skipped
        tag = pre + "loops/" + name
        fit = loops.fit_temperature(d, data, labs, 6, MEAN, STD, 25, **ckw, **kw)
        out[tag + "/fit"] = sha(sorted((k, np.float64(v).tobytes() if isinstance(v, float) else v) for k, v in fit.items()))
        out[tag + "/fit/beta_bits"] = int(np.float32(fit["beta"]).view(np.uint32))
        for form, skw in (("labels", dict()), ("scores", dict(score_maps=("entropy",))),
                          ("beta", dict(score_maps=KINDS, temperature_beta=fit["beta"]))):
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                res = loops.validate_test(d, data, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **ckw, **kw, **skw)
            out["%s/validate/%s/text" % (tag, form)] = sha(text.getvalue()) if rank0 else None
            out["%s/validate/%s/cm" % (tag, form)] = sha(res[0])
            out["%s/validate/%s/maps" % (tag, form)] = [sha(m) for m in res[1]]
            if skw:
                ex = res[2]
                out["%s/validate/%s/extra" % (tag, form)] = sha([
                    [sorted((k, sha(v)) for k, v in s.items()) for s in ex["scores"]], sha(ex["reliability"]),
                    sorted((k, repr(v)) for k, v in ex["calibration"].items()), ex.get("temperature_beta")])
        if "crop_sizes" in kw:
            continue
        for form, skw in (("labels", dict()), ("beta", dict(score_maps=KINDS, temperature_beta=fit["beta"]))):
            with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
                res = loops.generate_final_maps(d, data, ["7", "9"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", tmp + "/o_",
                                                **ckw, **kw, **skw)
                files = [(f, sha(open(os.path.join(tmp, f), "rb").read())) for f in sorted(os.listdir(tmp))]
            out["%s/final/%s/files" % (tag, form)] = sha(files) if rank0 else None
            out["%s/final/%s/n_files" % (tag, form)] = len(files) if rank0 else None
            maps = res[0] if skw else res
            out["%s/final/%s/maps" % (tag, form)] = [sha(m) for m in maps]
            if skw:
                out["%s/final/%s/scores" % (tag, form)] = sha([sorted((k, sha(v)) for k, v in s.items()) for s in res[1]])


def worker(rank, world, port, path):
    """one rank of `world` (1: no communicator); its digests go to <path>.<rank>"""
    out, comm = {}, None
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist
        from drs_amd.dist import TorchComm
        torch.cuda.set_device(0)
        comm = TorchComm("gloo")
    pre = "" if comm is None else "two_ranks/"
    predict_cases(out, comm, pre)
    loop_cases(out, comm, pre, paths=None if comm is None else ("windows", "dense_d4"))
    torch.cuda.synchronize()
    json.dump(out, open("%s.%d" % (path, rank), "w"))
    if comm is not None:
        comm.barrier()
        dist.destroy_process_group()


def main(out=None, ranks="2"):
    """the cases run in child processes, one after the other: this process never opens the GPU, so at most two hold it"""
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "r.json")
        mp.spawn(worker, args=(1, 0, path), nprocs=1, join=True)
        res.update(json.load(open(path + ".0")))
        if int(ranks) == 2:
            mp.spawn(worker, args=(2, 31500 + os.getpid() % 1000, path), nprocs=2, join=True)
            both = [json.load(open("%s.%d" % (path, r))) for r in range(2)]
            res.update(both[0])
            # what every rank holds whole must be the same on both (the text and the files are rank 0's)
            res["two_ranks/ranks_agree"] = all(both[1][k] == v for k, v in both[0].items() if v is not None and both[1][k] is not None)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(text + "\n")


if __name__ == "__main__":
    main(**dict(a.split("=", 1) for a in sys.argv[1:]))
