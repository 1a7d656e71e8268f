"""-m gpu: overlap-tile inference (loops.predict_tile_dense): the whole-tile forward of the net computed in tiles -- against the fp64
oracle on the whole tile in one piece, against one GPU forward of the whole tile, across tile sides, the receptive field it relies
on, the inference twin's weights, data parallelism and the process surface."""
import os
import random

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

from gpu_util import DEV, rel_err   # noqa: E402

CH, K = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])


def _net(net_type, b_max, s_max, seed=3, oracle=False):
    """a net with random moving statistics (eval-mode batch norm is then not the identity); and its fp64 oracle twin"""
    from drs_amd.net import DilatedNet
    rng = np.random.default_rng(seed)
    d = DilatedNet(net_type, CH, K, 0.005, b_max=b_max, s_max=s_max, device=DEV, seed=seed)
    o = T.OracleNet(net_type, CH, K, seed=seed) if oracle else None
    for n in d.variable_names():
        v = d.get_variable(n)
        if n.endswith("moving_mean"):
            v = (rng.normal(size=v.shape) * 0.1).astype(np.float32)
            d.set_variable(n, v)
        elif n.endswith("moving_variance"):
            v = rng.uniform(0.5, 2.0, size=v.shape).astype(np.float32)
            d.set_variable(n, v)
        if o is not None:
            o.p[n] = v.astype(np.float64)
    return d, o


def _tile(h, w, seed):
    from drs_amd.synthetic import make_tile
    return make_tile(h, w, CH, K, seed=seed, n_seeds=30)[0]


def _normalised(tile):
    x = tile.astype(np.float64).copy()
    x[..., :3] = (x[..., :3] - MEAN[:3]) / STD[:3]
    return x.astype(np.float32)          # what drs_crop_normalize writes: fp64 arithmetic, one rounding to fp32


def _dense(d, tile, bs, T_, sums=True):
    from drs_amd import loops, patches as P
    pool = P.TilePool([tile], None, DEV)
    h, w = tile.shape[:2]
    if sums:
        prob, occur, n = loops.predict_tile_dense(d, pool, 0, bs, MEAN, STD, tile=T_, return_sums=True)
        torch.cuda.synchronize()
        return prob.cpu().numpy().reshape(h, w, K), occur.cpu().numpy().reshape(h, w), n
    pred, n = loops.predict_tile_dense(d, pool, 0, bs, MEAN, STD, tile=T_)
    return pred.cpu().numpy(), n


def _clear(lg):
    srt = np.sort(lg, axis=-1)
    return (srt[..., -1] - srt[..., -2]) > 1e-3 * np.abs(lg).max()


@pytest.mark.parametrize("net_type", ["dilated_grsl_rate8", "dilated_grsl", "dilated_icpr_rate6_densely", "dilated_icpr_rate6_squeeze",
                                      "dilated_icpr_rate6_avgpool"])
def test_dense_tile_matches_oracle_whole_tile_forward(net_type):
    from drs_amd import patches as P
    h, w, T_, bs = 150, 230, 128, 4
    tile = _tile(h, w, seed=5)
    d, o = _net(net_type, 2, 24, oracle=True)
    prob, occur, n = _dense(d, tile, bs, T_)
    b, a = d.plan.receptive_field
    assert n == len(P.dense_tiles(h, w, T_, b, a)) and n > bs                        # several forwards per tile
    assert d._dense_twin.b_max == bs
    assert (occur == 1).all()
    ref = o.forward(_normalised(tile)[None].astype(np.float64), False)[0]         # the whole tile in one piece, fp64
    assert rel_err(prob, ref) <= 1e-4, rel_err(prob, ref)
    pred, _ = _dense(d, tile, bs, T_, sums=False)
    clear = _clear(ref)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(pred[clear], ref.argmax(-1)[clear])
    np.testing.assert_array_equal(pred, prob.argmax(-1))            # occur = 1: finalize is the plain first-maximum arg-max


def test_dense_equals_one_forward_of_the_whole_600_tile():
    from drs_amd import patches as P
    tile = _tile(600, 600, seed=6)
    d, _ = _net("dilated_grsl_rate8", 1, 600)
    pool = P.TilePool([tile], None, DEV)
    P.crop_to_net(d, pool, np.array([[0, 0, 0]]), 600, MEAN, STD)
    _, lg = d.forward(1, 600, want_logits=True)
    whole = lg[0].cpu().numpy().copy()
    for T_ in (512, 256):
        prob, occur, n = _dense(d, tile, 4, T_)
        assert (occur == 1).all() and n > 1
        assert rel_err(prob, whole) <= 1e-5, (T_, rel_err(prob, whole))
        pred, _ = _dense(d, tile, 4, T_, sums=False)
        clear = _clear(whole)
        assert clear.mean() > 0.9
        np.testing.assert_array_equal(pred[clear], whole.argmax(-1)[clear])


def test_dense_map_does_not_depend_on_the_tile_side():
    tile = _tile(300, 340, seed=7)
    d, _ = _net("dilated_grsl_rate8", 2, 24)
    res = {T_: _dense(d, tile, 4, T_) for T_ in (128, 160, 200)}
    ref = res[128][0]
    clear = _clear(ref)
    assert clear.mean() > 0.9
    for T_, (prob, occur, n) in res.items():
        assert (occur == 1).all()
        assert rel_err(prob, ref) <= 1e-5, (T_, rel_err(prob, ref))
        np.testing.assert_array_equal(prob.argmax(-1)[clear], ref.argmax(-1)[clear])


def test_receptive_field_bounds_the_reach_of_one_input_pixel():
    from drs_amd import known_net_types, resolve
    from drs_amd.nets import Plan
    S, q = 128, 64
    done = 0
    for t in sorted({resolve(n) for n in known_net_types()}):
        rf = Plan(t, CH, K).receptive_field
        if rf is None:
            continue
        b, a = rf
        d, _ = _net(t, 1, S)
        x = _normalised(_tile(S, S, seed=8))
        outs = []
        for bump in (0.0, 5.0):
            xx = x.copy()
            xx[q, q, :] += bump
            d.feed(xx.reshape(1, -1), None, S)
            _, lg = d.forward(1, S, want_logits=True)
            outs.append(lg[0].cpu().numpy().copy())
        changed = np.argwhere((outs[0] != outs[1]).any(-1))
        assert len(changed), t
        assert changed.min() >= q - a and changed.max() <= q + b, (t, rf, changed.min(0), changed.max(0))
        done += 1
        del d
    assert done >= 10


def test_dense_rejects_nets_with_squeeze_and_excitation():
    from drs_amd import loops, patches as P
    d, _ = _net("dilated_icpr_rate6_SE", 1, 24)
    pool = P.TilePool([_tile(64, 64, seed=9)], None, DEV)
    with pytest.raises(ValueError, match="squeeze-and-excitation"):
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=32)


def test_twin_follows_the_trained_net():
    d, _ = _net("dilated_icpr_rate6", 2, 24)
    tile = _tile(100, 120, seed=10)
    before, _, _ = _dense(d, tile, 2, 64)
    twin = d._dense_twin
    rng = np.random.default_rng(1)
    d.feed(rng.normal(size=(2, 24 * 24 * CH)).astype(np.float32), rng.integers(0, K, size=(2, 24 * 24)), 24)
    d.train_step(2, 24, 0.1)
    after, _, _ = _dense(d, tile, 2, 64)
    assert d._dense_twin is twin                 # cached ...
    d._dense_twin = None
    fresh, _, _ = _dense(d, tile, 2, 64)
    assert d._dense_twin is not twin
    np.testing.assert_array_equal(after, fresh)  # ... and fed the new weights on every call
    assert not np.array_equal(after, before)


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import loops, patches as P
    from drs_amd.dist import TorchComm
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    d, _ = _net("dilated_grsl", 1, 24)
    pool = P.TilePool([_tile(160, 150, seed=12)], None, DEV)
    pred, n = loops.predict_tile_dense(d, pool, 0, 1, MEAN, STD, comm=comm, tile=96)
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out, pred=pred.cpu().numpy(), n=n)
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_dense_map_equals_single_rank():
    import tempfile
    from drs_amd import patches as P
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dense_dp.npz")
        mp.spawn(_dp_worker, args=(2, 29700 + os.getpid() % 1000, out), nprocs=2, join=True)
        r = np.load(out)
        got, n = r["pred"], int(r["n"])
    d, _ = _net("dilated_grsl", 1, 24)
    tile = _tile(160, 150, seed=12)
    want, n1 = _dense(d, tile, 1, 96, sums=False)
    b, a = d.plan.receptive_field
    assert len(P.dense_axis(160, 96, b, a)[0]) >= 3 and n == n1
    np.testing.assert_array_equal(got, want)     # one tile per forward on both sides: the same launches, bitwise


def test_validate_test_and_cli_dense_tile(tmp_path, monkeypatch, capsys):
    from drs_amd import cli, loops, patches as P
    from drs_amd.net import DilatedNet
    # validate_test(dense_tile=...) scores the dense map
    d, _ = _net("dilated_grsl_rate8", 2, 24)
    tile = _tile(140, 150, seed=13)
    lab = np.random.default_rng(2).integers(0, 7, size=(140, 150)).astype(np.uint8)
    want, _ = _dense(d, tile, 4, 128, sums=False)
    cm, maps = loops.validate_test(d, [tile], [lab], ["t0"], 4, MEAN, STD, 25, 0, dense_tile=128)
    np.testing.assert_array_equal(maps[0], want)
    keep = lab != 6
    ref = np.zeros((K, K), dtype=np.int64)
    np.add.at(ref, (lab[keep], want[keep]), 1)
    np.testing.assert_array_equal(cm, ref)
    # the command line: train, then the maps with and without --dense-tile
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path) + "/out_"
    common = ["isprs_dilated_random.py", "synthetic:140x150x5/vaihingen/", out]
    tail = ["a", "c", "0.01", "0.005", "4", "2", "25", "10", "dilated8_grsl", "single_fixed", "25", "acc"]
    random.seed(0)
    np.random.seed(0)
    cli.main(common + ["none"] + tail + ["training"], device=DEV)
    capsys.readouterr()
    plain = cli.main(common + [out + "model-2"] + tail + ["generate_final_maps"], device=DEV)
    text_plain = capsys.readouterr().out
    dense = cli.main(["--dense-tile=128"] + common + [out + "model-2"] + tail + ["generate_final_maps"], device=DEV)
    text_dense = capsys.readouterr().out
    assert text_dense == text_plain and "--dense-tile" not in text_plain      # the flag is stripped before the parameters are printed
    np.testing.assert_array_equal(np.load(out + "top_mosaic_09cm_areac_class.npy"), dense[0])
    # the same maps from the loops, on the checkpoint the command line loaded
    net = DilatedNet("dilated8_grsl", CH, 6, 0.005, b_max=4, s_max=25, device=DEV)
    loops.load_checkpoint(net, out + "model-2")
    test_x, _ = cli.load_images("synthetic:140x150x5/vaihingen/", ["c"], "generate_final_maps")
    mean = np.load(os.path.join(str(tmp_path), "dataset_vaihingen_crop_25_stride_10_mean.npy"))
    std = np.load(os.path.join(str(tmp_path), "dataset_vaihingen_crop_25_stride_10_std.npy"))
    pool = P.TilePool(test_x, None, DEV)
    pd, _ = loops.predict_tile_dense(net, pool, 0, 4, mean, std, tile=128)
    np.testing.assert_array_equal(dense[0], pd.cpu().numpy())
    pw, _ = loops.predict_tile(net, pool, 0, 25, 4, mean, std)
    np.testing.assert_array_equal(plain[0], pw.cpu().numpy())             # without the flag: the sliding windows, as before
    assert not np.array_equal(plain[0], dense[0])
    cm2, maps2 = cli.main(common + [out + "model-2"] + tail + ["validate_test", "--dense-tile=128"], device=DEV)
    np.testing.assert_array_equal(maps2[0], dense[0])
