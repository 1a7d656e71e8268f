"""-m gpu: overlap-tile inference of the squeeze-and-excitation net with whole-image gates (loops.predict_tile_dense(se="global"),
DESIGN.md 8a.3) -- the three op-level pieces against numpy, the map against the fp64 oracle's forward of the whole image in one piece,
against one GPU forward of a one-tile image, across tile sides, run to run, with test-time augmentation and scales, on both twin
kinds, under data parallelism, and the process surface."""
import functools
import os
import random

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

import test_gpu_dense_predict as DP   # noqa: E402  (the nets, tiles and the clear-margin rule of the other dense tests)
import test_gpu_dense_scales as DS    # noqa: E402  (torch resize / normalise / softmax of the 8a.2 oracle statement)
from gpu_util import DEV, dev, rel_err, stream   # noqa: E402

CH, K, MEAN, STD = DP.CH, DP.K, DP.MEAN, DP.STD
SE_NET = "dilated_icpr_rate6_SE"
H, W, TT, BS = 150, 230, 128, 4


def _se_net(b_max=2, s_max=24, oracle=False):
    """the SE net as test_gpu_dense_predict._net builds it (random moving statistics), with fully connected SE weights large enough
    that the gates depend on the means (the initialiser's 0.005 leaves every gate at sigmoid(0.1) to four digits)"""
    d, o = DP._net(SE_NET, b_max, s_max, oracle=oracle)
    rng = np.random.default_rng(11)
    for n in d.variable_names():
        if "_fc" in n and n.endswith("/weights"):
            v = (rng.normal(size=d.get_variable(n).shape) * 0.3).astype(np.float32)
            d.set_variable(n, v)
            if o is not None:
                o.p[n] = v.astype(np.float64)
    return d, o


def _dense(d, tile, T_, bs=BS, sums=True, **kw):
    from drs_amd import loops, patches as P
    pool = P.TilePool([tile], None, DEV)
    h, w = tile.shape[:2]
    if sums:
        prob, occur, n = loops.predict_tile_dense(d, pool, 0, bs, MEAN, STD, tile=T_, return_sums=True, se="global", **kw)
        torch.cuda.synchronize()
        return prob.cpu().numpy().reshape(h, w, K), occur.cpu().numpy().reshape(h, w), n
    pred, n = loops.predict_tile_dense(d, pool, 0, bs, MEAN, STD, tile=T_, se="global", **kw)
    return pred.cpu().numpy(), n


@functools.lru_cache(maxsize=None)
def _oracle_logits(g=0, scale=None):
    """the fp64 oracle's eval forward of the whole (resized, transformed) image as ONE patch: its SE gates are whole-image means"""
    from drs_amd import patches as P
    _, o = _se_net(oracle=True)
    tile = DP._tile(H, W, seed=5)
    if scale is None:
        x = DP._normalised(tile).astype(np.float64)
    else:
        x = DS._normalise(DS._torch_resample(tile, P.scaled_size(H, scale), P.scaled_size(W, scale))).astype(np.float64)
    return o.forward(np.ascontiguousarray(P.dihedral_apply(x, g))[None], False)[0]


# ------------------------------------------------------------------------------------------------- the op-level pieces
def test_se_core_sums_against_numpy():
    from drs_amd import _lib
    rng = np.random.default_rng(0)
    for C_, T_, n in ((64, 40, 5), (256, 33, 4), (128, 128, 3)):
        act = rng.normal(size=(n, T_, T_, C_)).astype(np.float32) + 0.5
        boxes = np.array([[0, 0, 0, T_ - 7, 0, T_ - 5],                       # touching the top-left image border
                          [T_ - 10, 2 * T_, T_ - 3, 2 * T_ - 10, 2 * T_ + 6, 3 * T_],  # ... the right border (x0 + T = w)
                          [2 * T_, T_, 2 * T_ + 9, 3 * T_, T_ + 4, 2 * T_ - 4],        # ... the bottom border
                          [5, 7, 5, 5 + T_, 7, 7 + T_],                       # the whole tile
                          [10, 10, 12, 20, 30, 31]][:n], dtype=np.int32)      # one column
        boxes[n - 1] = [50, 60, 49, 60, 70, 75]                                # the last one's core starts above its tile: adds nothing
        want = np.full(C_, 3.25)
        for i, (y0, x0, cy0, cy1, cx0, cx1) in enumerate(boxes[:n - 1]):
            want += act[i, cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0].astype(np.float64).sum(axis=(0, 1))
        sums = torch.full((C_,), 3.25, dtype=torch.float64, device=DEV)        # the kernel ADDS
        scratch = torch.full((_lib.query("drs_se_core_sums_scratch_doubles", C_),), np.nan, dtype=torch.float64, device=DEV)
        a_d, b_d = dev(act), dev(boxes)
        _lib.call("drs_se_core_sums", a_d.data_ptr(), C_, T_, b_d.data_ptr(), n, sums.data_ptr(), scratch.data_ptr(), stream())
        torch.cuda.synchronize()
        got = sums.cpu().numpy()
        err = np.abs(got - want).max() / np.abs(want).max()
        print("se_core_sums C=%d T=%d n=%d: rel err %.3g" % (C_, T_, n, err))
        assert err <= 1e-12, (C_, T_, err)
        first = got.copy()
        sums.fill_(3.25)
        _lib.call("drs_se_core_sums", a_d.data_ptr(), C_, T_, b_d.data_ptr(), n, sums.data_ptr(), scratch.data_ptr(), stream())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(sums.cpu().numpy(), first)               # a fixed order: the same bits
    for bad in (dict(C=0), dict(T=0), dict(n=0)):
        a = dict(C=64, T=8, n=1)
        a.update(bad)
        assert _lib.query("drs_se_core_sums", a_d.data_ptr(), a["C"], a["T"], b_d.data_ptr(), a["n"], sums.data_ptr(), scratch.data_ptr(),
                          stream()) == 1


def test_se_gate_and_scale_const_against_the_oracle():
    from drs_amd import _lib
    rng = np.random.default_rng(1)
    B, S, C_, R, P_ = 3, 9, 128, 32, 4
    x = rng.normal(size=(1, 50, 70, C_)).astype(np.float32)
    w1, b1 = (rng.normal(size=(C_, R)) * 0.3).astype(np.float32), (rng.normal(size=R) * 0.1).astype(np.float32)
    w2, b2 = (rng.normal(size=(R, C_)) * 0.3).astype(np.float32), (rng.normal(size=C_) * 0.1).astype(np.float32)
    _, (s_ref, e1_ref, e2_ref) = T.se_forward(x.astype(np.float64), *[v.astype(np.float64) for v in (w1, b1, w2, b2)])
    sums = dev(x.astype(np.float64).sum(axis=(0, 1, 2)))
    s, e1, e2 = (torch.full((m,), np.nan, dtype=torch.float32, device=DEV) for m in (C_, R, C_))
    pd = [dev(v) for v in (w1, b1, w2, b2)]          # (kept alive until the launches have run)
    _lib.call("drs_se_gate", sums.data_ptr(), float(50 * 70), C_, R, pd[0].data_ptr(), pd[1].data_ptr(), pd[2].data_ptr(),
              pd[3].data_ptr(), s.data_ptr(), e1.data_ptr(), e2.data_ptr(), stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(s.cpu().numpy(), (x.astype(np.float64).sum(axis=(0, 1, 2)) / 3500.0).astype(np.float32))   # one rounding
    assert rel_err(e1.cpu().numpy(), e1_ref[0]) <= 1e-5 and rel_err(e2.cpu().numpy(), e2_ref[0]) <= 1e-5
    # one gate vector for the whole batch, halo zeroed, the slab's other channels untouched
    act = rng.normal(size=(B, S, S, C_)).astype(np.float32)
    ld, coff = C_ + 32, 32
    out = torch.full((B * (S + 2 * P_) ** 2 * ld,), 7.0, dtype=torch.float32, device=DEV)
    act_d = dev(act)
    _lib.call("drs_se_scale_const", act_d.data_ptr(), B, S, C_, e2.data_ptr(), out.data_ptr(), P_, ld, coff, stream())
    torch.cuda.synchronize()
    full = out.cpu().numpy().reshape(B, S + 2 * P_, S + 2 * P_, ld)
    np.testing.assert_array_equal(full[:, P_:P_ + S, P_:P_ + S, coff:], act * e2.cpu().numpy())
    assert (full[..., :coff] == 7.0).all()
    halo = full[..., coff:].copy()
    halo[:, P_:P_ + S, P_:P_ + S] = 0
    assert (halo == 0).all()


# ------------------------------------------------------------------------------------------------- the map
def test_global_se_map_matches_the_oracle_whole_image_forward():
    from drs_amd import patches as P
    tile = DP._tile(H, W, seed=5)
    d, _ = _se_net()
    prob, occur, n = _dense(d, tile, TT)
    assert d.plan.gated_receptive_field == (27, 28)
    assert n == len(P.dense_tiles(H, W, TT, 27, 28)) and n > BS          # several tiles, more tiles than the twin's batch
    assert d._dense_twin.b_max == BS
    assert (occur == 1).all()
    ref = _oracle_logits()
    print("se=global logits vs the oracle's whole-image forward: rel err %.3g" % rel_err(prob, ref))
    assert rel_err(prob, ref) <= 1e-4, rel_err(prob, ref)
    pred, _ = _dense(d, tile, TT, sums=False)
    clear = DP._clear(ref)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(pred[clear], ref.argmax(-1)[clear])
    np.testing.assert_array_equal(pred, prob.argmax(-1))
    # the gates are the oracle's whole-image gates
    _, o = _se_net(oracle=True)
    o.forward(DP._normalised(tile)[None].astype(np.float64), False)
    for j, li in enumerate(sorted(o.spec["se"])):
        e2 = o._se_cache[li][1][2][0]
        got = d._dense_twin.se_gate[j].cpu().numpy()
        assert np.ptp(e2) > 1e-3
        assert rel_err(got, e2) <= 1e-5, (j, rel_err(got, e2))


def test_one_tile_equals_the_forward_of_the_image_as_one_patch():
    from drs_amd import patches as P
    S = 96
    tile = DP._tile(S, S, seed=6)
    d, _ = _se_net(1, S)
    pool = P.TilePool([tile], None, DEV)
    P.crop_to_net(d, pool, np.array([[0, 0, 0]]), S, MEAN, STD)
    _, lg = d.forward(1, S, want_logits=True)            # the existing kernels: the patch mean IS the image mean here
    whole = lg[0].cpu().numpy().copy()
    prob, occur, n = _dense(d, tile, S)
    assert n == 1 and (occur == 1).all()
    print("one tile vs drs_forward of the image as one patch: rel err %.3g" % rel_err(prob, whole))
    assert rel_err(prob, whole) <= 1e-5, rel_err(prob, whole)


def test_map_does_not_depend_on_the_tile_side_and_repeats_bit_for_bit():
    tile = DP._tile(H, W, seed=5)
    d, _ = _se_net()
    a, occ_a, _ = _dense(d, tile, TT)
    gates = [g.clone() for g in d._dense_twin.se_gate]
    a2, _, _ = _dense(d, tile, TT)
    np.testing.assert_array_equal(a, a2)                                   # run twice: the same bits
    for g0, g1 in zip(gates, d._dense_twin.se_gate):
        assert torch.equal(g0, g1)
    b, occ_b, nb = _dense(d, tile, 96)
    assert (occ_a == 1).all() and (occ_b == 1).all() and nb > 6
    print("T = 96 against T = 128: rel err %.3g" % rel_err(b, a))
    assert rel_err(b, a) <= 1e-5, rel_err(b, a)
    # poisoned buffers: a map reads no sum or gate it has not written itself
    for t in d._dense_twin.se_sum + d._dense_twin.se_gate:
        t.fill_(float("nan"))
    a3, _, _ = _dense(d, tile, 96)
    np.testing.assert_array_equal(b, a3)


def _oracle_gates(g):
    """the oracle's SE gates when it is given the g-transformed whole image as one patch"""
    from drs_amd import patches as P
    _, o = _se_net(oracle=True)
    x = DP._normalised(DP._tile(H, W, seed=5)).astype(np.float64)
    o.forward(np.ascontiguousarray(P.dihedral_apply(x, g))[None], False)
    return [o._se_cache[li][1][2][0] for li in sorted(o.spec["se"])]


def test_tta_d4_matches_the_oracle_with_gates_per_code():
    """The net is not equivariant under the dihedral group (asymmetric SAME pads, unsymmetric filters), so the activation means -- and
    with them the gates -- of a flipped or rotated image are not those of the image.  Measured on one MI355X with gates taken once
    from the untransformed image: sums against the 8a.1 oracle statement 1.63e-4 (single codes: identity 3.6e-7, flips 1.9e-5 ..
    3.2e-5, transposed codes 3.2e-4 .. 3.4e-4), over the 1e-4 bound.  Every code therefore has gates of its own."""
    from drs_amd import patches as P
    tile = DP._tile(H, W, seed=5)
    d, _ = _se_net()
    _dense(d, tile, TT)
    plain = [g.clone() for g in d._dense_twin.se_gate]
    _dense(d, tile, TT, tta=(0,))                # the identity alone: the plain run's plan, sweeps and gates, bit for bit
    assert all(torch.equal(g0, g1) for g0, g1 in zip(plain, d._dense_twin.se_gate))
    for g in (2, 5):                             # a flip and a quarter-turn: the oracle's gates of the TRANSFORMED image
        _dense(d, tile, TT, tta=(g,))
        want = _oracle_gates(g)
        for j, e2 in enumerate(want):
            got = d._dense_twin.se_gate[j].cpu().numpy()
            print("code %d gate %d: rel err vs the oracle of the transformed image %.3g, vs the plain gates %.3g"
                  % (g, j, rel_err(got, e2), rel_err(plain[j].cpu().numpy(), e2)))
            assert rel_err(got, e2) <= 1e-5, (g, j, rel_err(got, e2))
    _dense(d, tile, TT, tta=(7,))
    last = [g.clone() for g in d._dense_twin.se_gate]
    acc, occur, n = _dense(d, tile, TT, tta="d4")
    assert (occur == 8).all() and n == len(P.dense_tiles(H, W, TT, 28, 28))      # the symmetric margin
    assert all(torch.equal(g0, g1) for g0, g1 in zip(last, d._dense_twin.se_gate))   # the buffers hold the last code's gates
    ref = sum(np.ascontiguousarray(P.dihedral_apply(DS._softmax(_oracle_logits(g)), g, inverse=True)) for g in range(8))
    print("tta=d4 sums vs the oracle: rel err %.3g" % rel_err(acc, ref))
    assert rel_err(acc, ref) <= 1e-4, rel_err(acc, ref)
    pred, _ = _dense(d, tile, TT, sums=False, tta="d4")
    clear = DP._clear(ref)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(pred[clear], ref.argmax(-1)[clear])


def test_scales_with_flip_match_the_oracle():
    from drs_amd import patches as P
    tile = DP._tile(H, W, seed=5)
    d, _ = _se_net()
    acc, occur, _ = _dense(d, tile, 96, scales=(1.25,), tta=(0, 6))
    ref = sum(DS._torch_resample(np.ascontiguousarray(P.dihedral_apply(DS._softmax(_oracle_logits(g, 1.25)), g, inverse=True)), H, W)
              for g in (0, 6)) / 2
    assert (occur == 1).all()
    print("scales=(1.25,) with tta=(0, 6) vs the oracle: rel err %.3g" % rel_err(acc, ref))
    assert rel_err(acc, ref) <= 1e-4, rel_err(acc, ref)


def test_scales_match_the_oracle():
    from drs_amd import patches as P
    tile = DP._tile(H, W, seed=5)
    d, _ = _se_net()
    scales = (0.75, 1.25)
    acc, occur, n = _dense(d, tile, 96, scales=scales)
    assert (occur == 2).all()
    assert n == sum(len(P.dense_tiles(P.scaled_size(H, s), P.scaled_size(W, s), 96, 27, 28)) for s in scales)
    ref = sum(DS._torch_resample(DS._softmax(_oracle_logits(0, s)), H, W) for s in scales)
    print("scales=(0.75, 1.25) sums vs the oracle: rel err %.3g" % rel_err(acc, ref))
    assert rel_err(acc, ref) <= 1e-4, rel_err(acc, ref)


def test_both_twin_kinds_give_the_same_bits(monkeypatch):
    from drs_amd.engine import EngineNet
    from drs_amd.oplevel import OpLevelNet
    tile = DP._tile(H, W, seed=5)
    d, _ = _se_net()
    a, _, _ = _dense(d, tile, TT)
    assert isinstance(d._dense_twin, EngineNet)
    monkeypatch.setenv("DRS_OP_LEVEL", "1")
    d2, _ = _se_net()
    b, occur, _ = _dense(d2, tile, TT)
    assert isinstance(d2, OpLevelNet) and isinstance(d2._dense_twin, OpLevelNet)
    assert (occur == 1).all()
    np.testing.assert_array_equal(a, b)          # the same launches in the same order
    for g0, g1 in zip(d._dense_twin.se_gate, d2._dense_twin.se_gate):
        assert torch.equal(g0, g1)


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import loops, patches as P
    from drs_amd.dist import TorchComm
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    d, _ = _se_net(1, 24)
    pool = P.TilePool([DP._tile(H, W, seed=5)], None, DEV)
    prob, occur, n = loops.predict_tile_dense(d, pool, 0, BS, MEAN, STD, comm=comm, tile=96, return_sums=True, se="global")
    pred, _ = loops.predict_tile_dense(d, pool, 0, BS, MEAN, STD, comm=comm, tile=96, se="global")
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out, prob=prob.cpu().numpy(), occur=occur.cpu().numpy(), pred=pred.cpu().numpy(), n=n)
    comm.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_against_one_rank():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dense_se_dp.npz")
        mp.spawn(_dp_worker, args=(2, 29700 + os.getpid() % 1000, out), nprocs=2, join=True)
        r = np.load(out)
        prob2, occur2, pred2, n2 = r["prob"].reshape(H, W, K), r["occur"].reshape(H, W), r["pred"], int(r["n"])
    d, _ = _se_net(1, 24)
    tile = DP._tile(H, W, seed=5)
    prob1, occur1, n1 = _dense(d, tile, 96)
    pred1, _ = _dense(d, tile, 96, sums=False)
    assert n1 == n2 and (occur2 == 1).all() and (occur1 == 1).all()
    print("two ranks against one rank: rel err of the sums %.3g" % rel_err(prob2, prob1))
    assert rel_err(prob2, prob1) <= 1e-5, rel_err(prob2, prob1)       # (the cross-rank fp64 sum changes the order: not bitwise)
    clear = DP._clear(prob1)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(pred2[clear], pred1[clear])


def test_se_mode_is_refused_where_it_means_nothing_and_the_default_still_raises():
    from drs_amd import loops, patches as P
    pool = P.TilePool([DP._tile(64, 64, seed=9)], None, DEV)
    d, _ = DP._net("dilated_grsl_rate8", 1, 24)
    with pytest.raises(ValueError, match="no squeeze-and-excitation"):
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=32, se="global")
    d, _ = _se_net(1, 24)
    with pytest.raises(ValueError, match="squeeze-and-excitation"):
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=32)
    with pytest.raises(ValueError, match="se must be"):
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=32, se="local")
    assert d.plan.receptive_field is None


def test_validate_test_and_cli_dense_se(tmp_path, monkeypatch, capsys):
    from drs_amd import cli, loops
    from drs_amd.net import DilatedNet
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path) + "/out_"
    common = ["isprs_dilated_random.py", "synthetic:140x150x5/vaihingen/", out]
    tail = ["a", "c", "0.01", "0.005", "4", "2", "25", "10", SE_NET, "single_fixed", "25", "acc"]
    random.seed(0)
    np.random.seed(0)
    cli.main(common + ["none"] + tail + ["training"], device=DEV)
    capsys.readouterr()
    with pytest.raises(ValueError, match="squeeze-and-excitation"):
        cli.main(common + [out + "model-2"] + tail + ["validate_test", "--dense-tile=128"], device=DEV)
    capsys.readouterr()
    cm, maps = cli.main(common + [out + "model-2"] + tail + ["validate_test", "--dense-tile=128", "--dense-se=global"], device=DEV)
    text = capsys.readouterr().out
    assert "--dense-se" not in text                                   # the flag is stripped before the parameters are printed
    assert "-- Test Map c: Overall Accuracy= " in text and "-- Test ALL MAPS: Overall Accuracy= " in text
    assert " Confusion Matrix= " in text and " Mean Kappa Score= " in text
    # the same from the library, on the checkpoint the command line loaded
    net = DilatedNet(SE_NET, CH, 6, 0.005, b_max=4, s_max=25, device=DEV)
    loops.load_checkpoint(net, out + "model-2")
    test_x, test_y = cli.load_images("synthetic:140x150x5/vaihingen/", ["c"], "validate_test")
    mean = np.load(os.path.join(str(tmp_path), "dataset_vaihingen_crop_25_stride_10_mean.npy"))
    std = np.load(os.path.join(str(tmp_path), "dataset_vaihingen_crop_25_stride_10_std.npy"))
    cm2, maps2 = loops.validate_test(net, test_x, test_y, ["c"], 4, mean, std, 25, 2, dense_tile=128, dense_se="global")
    np.testing.assert_array_equal(cm, cm2)
    np.testing.assert_array_equal(maps[0], maps2[0])
    assert cm.sum() > 0
