"""-m gpu: dihedral test-time augmentation of overlap-tile inference (loops.predict_tile_dense(..., tta=...)) -- the two kernels bit for
bit / against numpy, every single code against the fp64 oracle's whole-image forward of the transformed image (which tells the two
quarter-turns apart), the "flip" and "d4" means, equivariance, independence from the tile side, data parallelism and the process
surface."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

from gpu_util import DEV, rel_err, stream   # noqa: E402

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
    return x.astype(np.float32)


def _softmax(lg):
    e = np.exp(lg - lg.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _tta(d, tile, bs, T_, tta, sums=True):
    from drs_amd import loops, patches as P
    pool = P.TilePool([tile], None, DEV)
    h, w = tile.shape[:2]
    if sums:
        acc, occur, n = loops.predict_tile_dense(d, pool, 0, bs, MEAN, STD, tile=T_, return_sums=True, tta=tta)
        torch.cuda.synchronize()
        return acc.cpu().numpy().reshape(h, w, K), occur.cpu().numpy().reshape(h, w), n
    pred, n = loops.predict_tile_dense(d, pool, 0, bs, MEAN, STD, tile=T_, tta=tta)
    return pred.cpu().numpy(), n


def _clear(p):
    srt = np.sort(p, axis=-1)
    return (srt[..., -1] - srt[..., -2]) > 1e-3 * np.abs(p).max()


# ------------------------------------------------------------------------------------------------------------ the crop kernel
def _crop_pair(pool, inst, T_, P_, ld, g=None, flip=None, fill=np.nan):
    """one call of drs_crop_dihedral (g) or of drs_crop_normalize (flip, no augmentation) into a slab pre-filled with `fill`"""
    from drs_amd import _lib
    B = len(inst)
    out = torch.full((B * (T_ + 2 * P_) ** 2 * ld,), float(fill), dtype=torch.float32, device=DEV)
    m3, s3 = (C.c_double * 3)(*MEAN[:3]), (C.c_double * 3)(*STD[:3])
    if g is not None:
        dinst = torch.tensor(np.asarray(inst, dtype=np.int32)[:, :3].copy(), device=DEV)
        _lib.call("drs_crop_dihedral", pool.tiles.data_ptr(), 1 if pool.f64 else 0, pool.tile_off.data_ptr(), pool.tile_h.data_ptr(),
                  pool.tile_w.data_ptr(), len(pool.h), CH, dinst.data_ptr(), g, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), B, T_,
                  P_, ld, out.data_ptr(), stream())
    else:
        i4 = np.zeros((B, 4), dtype=np.int32)
        i4[:, :3] = np.asarray(inst)[:, :3]
        i4[:, 3] = flip
        dinst = torch.tensor(i4, device=DEV)
        _lib.call("drs_crop_normalize", pool.tiles.data_ptr(), 1 if pool.f64 else 0, pool.labels.data_ptr(), pool.tile_off.data_ptr(),
                  pool.lab_off.data_ptr(), pool.tile_h.data_ptr(), pool.tile_w.data_ptr(), CH, dinst.data_ptr(), None, None, None, None,
                  0, 0, C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), B, T_, P_, ld, out.data_ptr(), None, None, -1, 0, stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(B, T_ + 2 * P_, T_ + 2 * P_, ld)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T_", [128, 77])
def test_crop_dihedral_bitwise(T_, dtype):
    from drs_amd import patches as P
    tiles = [_tile(200, 170, seed=20), _tile(T_ + 3, 260, seed=21)]
    pool = P.TilePool(tiles, None, DEV, dtype=dtype)
    inst = np.array([[0, 0, 0], [0, 200 - T_, 170 - T_], [1, 2, 91], [0, 31, 17]])
    P_, ld = 3, 8
    base = _crop_pair(pool, inst, T_, P_, ld, flip=0)
    assert not np.isnan(base).any()
    interior = base[:, P_:P_ + T_, P_:P_ + T_]
    want0 = np.zeros_like(base)
    for b, (m, r, c) in enumerate(inst):
        x = tiles[m][r:r + T_, c:c + T_].astype(dtype).astype(np.float64)
        x[..., :3] = (x[..., :3] - MEAN[:3]) / STD[:3]
        want0[b, P_:P_ + T_, P_:P_ + T_, :CH] = x.astype(np.float32)
    np.testing.assert_array_equal(base, want0)                  # the reference normalisation, one rounding, zero halo / padding
    for g in range(8):
        got = _crop_pair(pool, inst, T_, P_, ld, g=g)
        want = np.zeros_like(base)
        want[:, P_:P_ + T_, P_:P_ + T_] = np.stack([P.dihedral_apply(interior[b], g) for b in range(len(inst))])
        np.testing.assert_array_equal(got, want, err_msg="g=%d" % g)      # the sigma_g permutation of the g = 0 slab, bit for bit
        if g == 0:
            np.testing.assert_array_equal(got, base)
    np.testing.assert_array_equal(_crop_pair(pool, inst, T_, P_, ld, g=2), _crop_pair(pool, inst, T_, P_, ld, flip=1))   # flipud
    np.testing.assert_array_equal(_crop_pair(pool, inst, T_, P_, ld, g=1), _crop_pair(pool, inst, T_, P_, ld, flip=2))   # fliplr


def test_crop_dihedral_zeroes_tiles_outside_their_map():
    from drs_amd import patches as P
    T_ = 64
    tiles = [_tile(100, 90, seed=22), _tile(70, 80, seed=23)]
    pool = P.TilePool(tiles, None, DEV, dtype=np.float32)
    bad = [[0, 100 - T_ + 1, 0], [0, 0, 90 - T_ + 1], [0, -1, 0], [1, 0, -3], [1, 7, 0], [2, 0, 0], [-1, 0, 0]]
    inst = np.array([[1, 6, 16]] + bad + [[0, 36, 26]])
    for g in (0, 5, 6):
        got = _crop_pair(pool, inst, T_, 2, 8, g=g, fill=7.0)
        assert (got[1:-1] == 0).all(), g
        want = _crop_pair(pool, inst[[0, -1]], T_, 2, 8, g=g)
        np.testing.assert_array_equal(got[[0, -1]], want)


# ------------------------------------------------------------------------------------------------------------ the place kernel
def test_tile_place_dihedral_against_numpy():
    from drs_amd import _lib, patches as P
    h, w, T_, m = 150, 230, 128, 51
    boxes = P.dense_tiles(h, w, T_, m, m)
    n = len(boxes)
    rng = np.random.default_rng(4)
    logits = (rng.normal(size=(n, T_, T_, K)) * 4).astype(np.float32)
    lg_dev = torch.from_numpy(logits).to(DEV)
    bx_dev = torch.from_numpy(boxes.astype(np.int32)).to(DEV)
    acc0 = rng.uniform(0, 2, size=(h, w, K)).astype(np.float32)
    for g in range(8):
        acc = torch.from_numpy(acc0.copy()).to(DEV)
        occur = torch.zeros(h * w, dtype=torch.int32, device=DEV)
        _lib.call("drs_tile_place_dihedral", acc.data_ptr(), occur.data_ptr(), lg_dev.data_ptr(), h, w, K, T_, bx_dev.data_ptr(), n, g,
                  stream())
        torch.cuda.synchronize()
        want = acc0.astype(np.float64).copy()
        (_, _), (Ii, Ji) = P.dihedral_index(g, T_)
        for i, (y0, x0, cy0, cy1, cx0, cx1) in enumerate(boxes):
            back = _softmax(logits[i].astype(np.float64)[Ii, Ji])            # the logits of the transformed tile on the tile's grid
            want[cy0:cy1, cx0:cx1] += back[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
        got = acc.cpu().numpy()
        assert rel_err(got, want) <= 1e-6, (g, rel_err(got, want))
        assert (occur.cpu().numpy() == 1).all(), g


# ------------------------------------------------------------------------------------------------------------ against the oracle
H, W, TT, BS = 150, 230, 128, 4
NETS = ["dilated_grsl_rate8", "dilated_grsl", "dilated_icpr_rate6_densely", "dilated_icpr_rate6_avgpool"]


@functools.lru_cache(maxsize=None)
def _oracle_views(net_type):
    """softmax(F(g . X)) put back on X's grid by g^-1, for g = 0..7: F = the fp64 oracle's whole-image eval forward"""
    from drs_amd import patches as P
    _, o = _net(net_type, 2, 24, oracle=True)        # the same construction as the tests' nets
    x = _normalised(_tile(H, W, seed=5)).astype(np.float64)
    out = []
    for g in range(8):
        lg = o.forward(np.ascontiguousarray(P.dihedral_apply(x, g))[None], False)[0]
        out.append(np.ascontiguousarray(P.dihedral_apply(_softmax(lg), g, inverse=True)))
    return out


@pytest.mark.parametrize("net_type", NETS)
def test_every_single_code_matches_the_oracle_of_the_transformed_image(net_type):
    d, _ = _net(net_type, 2, 24)
    tile = _tile(H, W, seed=5)
    ref = _oracle_views(net_type)
    for g in range(8):
        acc, occur, n = _tta(d, tile, BS, TT, (g,))
        assert (occur == 1).all(), g
        assert n > BS
        assert rel_err(acc, ref[g]) <= 1e-4, (net_type, g, rel_err(acc, ref[g]))
        if g in (5, 6):           # the two quarter-turns are each other's inverse: the test tells them apart
            assert rel_err(acc, ref[11 - g]) > 1e-3, (net_type, g)


@pytest.mark.parametrize("group", ["flip", "d4"])
def test_groups_match_the_oracle_mean(group):
    from drs_amd import patches as P
    net_type = "dilated_grsl_rate8"
    d, _ = _net(net_type, 2, 24)
    tile = _tile(H, W, seed=5)
    G = P.tta_group(group)
    ref = sum(_oracle_views(net_type)[g] for g in G)
    acc, occur, n = _tta(d, tile, BS, TT, group)
    assert (occur == len(G)).all()
    assert rel_err(acc, ref) <= 1e-4, rel_err(acc, ref)
    pred, n2 = _tta(d, tile, BS, TT, group, sums=False)
    assert n2 == n
    clear = _clear(ref)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(pred[clear], ref.argmax(-1)[clear])
    if group == "flip":
        acc2, occur2, _ = _tta(d, tile, BS, TT, (3, 1, 0, 2))
        np.testing.assert_array_equal(acc2, acc)
        np.testing.assert_array_equal(occur2, occur)
    # the plain map is another function: TTA is not a no-op
    plain, _, _ = _tta(d, tile, BS, TT, None)
    assert rel_err(_softmax(plain.astype(np.float64)) * len(G), acc) > 1e-3


# ------------------------------------------------------------------------------------------------------------ properties of the map
def test_equivariance_under_transpose_and_flipud():
    d, _ = _net("dilated_grsl_rate8", 2, 24)
    tile = _tile(H, W, seed=6)
    a, _, _ = _tta(d, tile, BS, TT, "d4")
    b, _, _ = _tta(d, np.ascontiguousarray(tile.swapaxes(0, 1)), BS, TT, "d4")
    assert rel_err(b, a.swapaxes(0, 1)) <= 1e-5, rel_err(b, a.swapaxes(0, 1))
    a, _, _ = _tta(d, tile, BS, TT, "flip")
    b, _, _ = _tta(d, np.ascontiguousarray(tile[::-1]), BS, TT, "flip")
    assert rel_err(b, a[::-1]) <= 1e-5, rel_err(b, a[::-1])


def test_tta_map_does_not_depend_on_the_tile_side():
    d, _ = _net("dilated_grsl_rate8", 2, 24)
    tile = _tile(260, 300, seed=7)
    res = {T_: _tta(d, tile, 4, T_, "d4") for T_ in (128, 160, 200)}
    ref = res[128][0]
    for T_, (acc, occur, n) in res.items():
        assert (occur == 8).all()
        assert rel_err(acc, ref) <= 1e-5, (T_, rel_err(acc, ref))
    again, _, _ = _tta(d, tile, 4, 160, "d4")
    np.testing.assert_array_equal(again, res[160][0])           # deterministic: no float atomics


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import loops, patches as P
    from drs_amd.dist import TorchComm
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    d, _ = _net("dilated_grsl", 1, 24)
    pool = P.TilePool([_tile(160, 150, seed=12)], None, DEV)
    pred, n = loops.predict_tile_dense(d, pool, 0, 1, MEAN, STD, comm=comm, tile=96, tta="d4")
    acc, occur, _ = loops.predict_tile_dense(d, pool, 0, 1, MEAN, STD, comm=comm, tile=96, tta="d4", return_sums=True)
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out, pred=pred.cpu().numpy(), n=n, acc=acc.cpu().numpy(), occur=occur.cpu().numpy())
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_tta_map_equals_single_rank():
    import tempfile
    from drs_amd import patches as P
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tta_dp.npz")
        mp.spawn(_dp_worker, args=(2, 29800 + os.getpid() % 1000, out), nprocs=2, join=True)
        r = np.load(out)
        got, n, acc, occur = r["pred"], int(r["n"]), r["acc"], r["occur"]
    d, _ = _net("dilated_grsl", 1, 24)
    tile = _tile(160, 150, seed=12)
    want, n1 = _tta(d, tile, 1, 96, "d4", sums=False)
    wacc, woccur, _ = _tta(d, tile, 1, 96, "d4")
    m = max(d.plan.receptive_field)
    assert len(P.dense_axis(160, 96, m, m)[0]) >= 3 and n == n1
    np.testing.assert_array_equal(got, want)     # one tile per forward on both sides: the same launches, bitwise
    np.testing.assert_array_equal(occur.reshape(160, 150), woccur)
    np.testing.assert_array_equal(acc.reshape(160, 150, K), wacc)


# ------------------------------------------------------------------------------------------------------------ the process surface
def test_tta_rejects_nets_with_squeeze_and_excitation_and_bad_groups():
    from drs_amd import loops, patches as P
    d, _ = _net("dilated_icpr_rate6_SE", 1, 24)
    pool = P.TilePool([_tile(64, 64, seed=9)], None, DEV)
    with pytest.raises(ValueError, match="squeeze-and-excitation"):
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=32, tta="d4")
    d, _ = _net("dilated_grsl", 1, 24)
    for bad in ("rot90", (8,), (1, 1)):
        with pytest.raises(ValueError):
            loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=64, tta=bad)


def test_validate_test_and_cli_dense_tta(tmp_path, monkeypatch, capsys):
    from drs_amd import cli, loops, patches as P
    from drs_amd.net import DilatedNet
    d, _ = _net("dilated_grsl_rate8", 2, 24)
    tile = _tile(140, 150, seed=13)
    lab = np.random.default_rng(2).integers(0, 7, size=(140, 150)).astype(np.uint8)
    want, _ = _tta(d, tile, 4, 128, "d4", sums=False)
    cm, maps = loops.validate_test(d, [tile], [lab], ["t0"], 4, MEAN, STD, 25, 0, dense_tile=128, dense_tta="d4")
    np.testing.assert_array_equal(maps[0], want)
    keep = lab != 6
    ref = np.zeros((K, K), dtype=np.int64)
    np.add.at(ref, (lab[keep], want[keep]), 1)
    np.testing.assert_array_equal(cm, ref)
    # the command line: train, then the maps with and without the flags
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
    tta = cli.main(["--dense-tta=d4"] + common + [out + "model-2"] + tail + ["generate_final_maps", "--dense-tile=128"], device=DEV)
    text_tta = capsys.readouterr().out
    assert text_tta == text_plain and "--dense-t" not in text_plain      # both flags are stripped before the parameters are printed
    np.testing.assert_array_equal(np.load(out + "top_mosaic_09cm_areac_class.npy"), tta[0])
    net = DilatedNet("dilated8_grsl", CH, 6, 0.005, b_max=4, s_max=25, device=DEV)
    loops.load_checkpoint(net, out + "model-2")
    test_x, _ = cli.load_images("synthetic:140x150x5/vaihingen/", ["c"], "generate_final_maps")
    mean = np.load(os.path.join(str(tmp_path), "dataset_vaihingen_crop_25_stride_10_mean.npy"))
    std = np.load(os.path.join(str(tmp_path), "dataset_vaihingen_crop_25_stride_10_std.npy"))
    pool = P.TilePool(test_x, None, DEV)
    pd, _ = loops.predict_tile_dense(net, pool, 0, 4, mean, std, tile=128, tta="d4")
    np.testing.assert_array_equal(tta[0], pd.cpu().numpy())
    pw, _ = loops.predict_tile(net, pool, 0, 25, 4, mean, std)
    np.testing.assert_array_equal(plain[0], pw.cpu().numpy())             # without the flags: the sliding windows, as before
    cm2, maps2 = cli.main(common + [out + "model-2"] + tail + ["validate_test", "--dense-tile=128", "--dense-tta=d4"], device=DEV)
    np.testing.assert_array_equal(maps2[0], tta[0])
    with pytest.raises(SystemExit) as e:
        cli.main(common + [out + "model-2"] + tail + ["validate_test", "--dense-tta=d4"], device=DEV)
    assert "--dense-tile" in str(e.value)
