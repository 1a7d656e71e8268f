"""-m gpu: multi-scale test-time augmentation of overlap-tile inference (loops.predict_tile_dense(..., scales=...)) -- the resampling crop
against torch's fp64 resize and bit for bit against drs_crop_dihedral at scale 1, the resample-accumulate kernel against the numpy
statement of the bilinear rule, every single scale and their sum against the fp64 oracle's whole-image forward of the resized image,
with D4 too, the scale-1 identities, independence from the tile side, the twin sized once, data parallelism and the process surface."""
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
from test_dense_scales_plan import _torch_resample, resample   # noqa: E402  (the numpy statement of the bilinear rule)

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


def _normalise(x):
    """fp64 in, the normalisation of drs_crop_normalize (bands 0..2), one rounding to fp32"""
    x = np.asarray(x, dtype=np.float64).copy()
    x[..., :3] = (x[..., :3] - MEAN[:3]) / STD[:3]
    return x.astype(np.float32)


def _softmax(lg):
    e = np.exp(lg - lg.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _clear(p):
    srt = np.sort(p, axis=-1)
    return (srt[..., -1] - srt[..., -2]) > 1e-3 * np.abs(p).max()


def _dense(d, tile, bs, T_, scales, tta=None, sums=True):
    from drs_amd import loops, patches as P
    pool = P.TilePool([tile], None, DEV)
    h, w = tile.shape[:2]
    if sums:
        acc, occur, n = loops.predict_tile_dense(d, pool, 0, bs, MEAN, STD, tile=T_, return_sums=True, tta=tta, scales=scales)
        torch.cuda.synchronize()
        return acc.cpu().numpy().reshape(h, w, K), occur.cpu().numpy().reshape(h, w), n
    pred, n = loops.predict_tile_dense(d, pool, 0, bs, MEAN, STD, tile=T_, tta=tta, scales=scales)
    return pred.cpu().numpy(), n


# ------------------------------------------------------------------------------------------------------------ the crop kernel
def _m3s3():
    return (C.c_double * 3)(*MEAN[:3]), (C.c_double * 3)(*STD[:3])


def _crop(pool, inst, T_, P_, ld, g, hs=None, ws=None, fill=np.nan):
    """one call of drs_crop_resampled (hs, ws given) or of drs_crop_dihedral into a slab pre-filled with `fill`"""
    from drs_amd import _lib
    B = len(inst)
    out = torch.full((B * (T_ + 2 * P_) ** 2 * ld,), float(fill), dtype=torch.float32, device=DEV)
    m3, s3 = _m3s3()
    dinst = torch.tensor(np.asarray(inst, dtype=np.int32)[:, :3].copy(), device=DEV)
    head = (pool.tiles.data_ptr(), 1 if pool.f64 else 0, pool.tile_off.data_ptr(), pool.tile_h.data_ptr(), pool.tile_w.data_ptr(),
            len(pool.h), CH, dinst.data_ptr())
    tail = (C.cast(m3, C.c_void_p), C.cast(s3, C.c_void_p), B, T_, P_, ld, out.data_ptr(), stream())
    if hs is None:
        _lib.call("drs_crop_dihedral", *head, g, *tail)
    else:
        _lib.call("drs_crop_resampled", *head, hs, ws, g, *tail)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(B, T_ + 2 * P_, T_ + 2 * P_, ld)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_crop_resampled_matches_torch_resize_then_crop(dtype):
    from drs_amd import patches as P
    tiles = [_tile(90, 110, seed=30), _tile(70, 64, seed=31)]
    pool = P.TilePool(tiles, None, DEV, dtype=dtype)
    T_, P_, ld = 48, 3, 8
    for hs, ws in ((135, 165), (60, 70), (101, 83), (90, 231)):
        scaled = [_normalise(_torch_resample(t.astype(dtype), hs, ws)) for t in tiles]     # each map resampled to hs x ws
        inst = np.array([[0, 0, 0], [0, hs - T_, ws - T_], [1, (hs - T_) // 2, 5], [1, 3, ws - T_ - 1], [0, 7, (ws - T_) // 3]])
        for g in range(8):
            got = _crop(pool, inst, T_, P_, ld, g, hs, ws)
            assert not np.isnan(got).any()
            want = np.zeros_like(got)
            for b, (m, r, c) in enumerate(inst):
                want[b, P_:P_ + T_, P_:P_ + T_, :CH] = P.dihedral_apply(scaled[m][r:r + T_, c:c + T_], g)
            zero = want == 0
            assert (got[zero] == 0).all(), (hs, ws, g)                   # halo and channels C..ld-1
            assert rel_err(got, want) <= 1e-6, (hs, ws, g, rel_err(got, want))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_crop_resampled_at_scale_one_is_crop_dihedral_bitwise(dtype):
    from drs_amd import patches as P
    tiles = [_tile(90, 110, seed=32), _tile(77, 64, seed=33)]
    pool = P.TilePool(tiles, None, DEV, dtype=dtype)
    T_, P_, ld = 64, 2, 8
    inst = np.array([[0, 0, 0], [0, 90 - T_, 110 - T_], [0, 11, 29], [0, 5, 46]])
    for g in range(8):
        want = _crop(pool, inst, T_, P_, ld, g)
        np.testing.assert_array_equal(_crop(pool, inst, T_, P_, ld, g, 90, 110), want, err_msg="g=%d" % g)
    inst = np.array([[1, 0, 0], [1, 13, 0]])                             # the second map at its own size
    for g in (0, 5, 6):
        np.testing.assert_array_equal(_crop(pool, inst, T_, P_, ld, g, 77, 64), _crop(pool, inst, T_, P_, ld, g), err_msg="g=%d" % g)


def test_crop_resampled_zeroes_tiles_outside_the_scaled_grid():
    from drs_amd import patches as P
    T_, hs, ws = 40, 120, 96                           # map 0 is 100 x 90; the call's grid is 120 x 96
    tiles = [_tile(100, 90, seed=34), _tile(70, 80, seed=35)]
    pool = P.TilePool(tiles, None, DEV, dtype=np.float32)
    bad = [[0, hs - T_ + 1, 0], [0, 0, ws - T_ + 1], [0, -1, 0], [1, 0, -3], [2, 0, 0], [-1, 0, 0]]
    inst = np.array([[1, 6, 16]] + bad + [[0, hs - T_, ws - T_]])
    for g in (0, 5, 6):
        got = _crop(pool, inst, T_, 2, 8, g, hs, ws, fill=7.0)
        assert (got[1:-1] == 0).all(), g
        want = _crop(pool, inst[[0, -1]], T_, 2, 8, g, hs, ws)
        np.testing.assert_array_equal(got[[0, -1]], want)


# ------------------------------------------------------------------------------------------------------------ the resample kernel
def _accumulate(src, occur, K_, is_prob, h, w, acc0):
    from drs_amd import _lib
    hs, ws = occur.shape
    acc = torch.from_numpy(acc0.copy()).to(DEV)
    s_dev, o_dev = torch.from_numpy(np.ascontiguousarray(src)).to(DEV), torch.from_numpy(occur.astype(np.int32)).to(DEV)
    _lib.call("drs_resample_accumulate", s_dev.data_ptr(), o_dev.data_ptr(), hs, ws, K_, int(is_prob), h, w, acc.data_ptr(), stream())
    torch.cuda.synchronize()
    return acc.cpu().numpy()


@pytest.mark.parametrize("is_prob", [1, 0])
def test_resample_accumulate_against_numpy(is_prob):
    rng = np.random.default_rng(8)
    for (hs, ws), (h, w) in (((50, 70), (80, 95)), ((120, 130), (80, 95)), ((33, 200), (61, 47)), ((1, 9), (4, 4))):
        occur = rng.integers(0, 9 if is_prob else 3, size=(hs, ws))
        src = (rng.uniform(0, 1, size=(hs, ws, K)) * np.maximum(occur, 1)[..., None] if is_prob
               else rng.normal(size=(hs, ws, K)) * 4).astype(np.float32)
        acc0 = rng.uniform(0, 2, size=(h, w, K)).astype(np.float32)
        vec = src.astype(np.float64) / np.maximum(occur, 1)[..., None]
        if not is_prob:
            vec = _softmax(vec)
        want = acc0 + resample(vec, h, w)
        got = _accumulate(src, occur, K, is_prob, h, w, acc0)
        assert rel_err(got, want) <= 1e-6, ((hs, ws), (h, w), rel_err(got, want))


def test_resample_accumulate_at_equal_sizes_is_acc_plus_the_vector_bitwise():
    from drs_amd import _lib
    rng = np.random.default_rng(9)
    h = w = 64
    acc0 = rng.uniform(0, 2, size=(h, w, K)).astype(np.float32)
    occur = rng.integers(0, 9, size=(h, w))
    src = (rng.uniform(0, 1, size=(h, w, K)) * 8).astype(np.float32)
    want = acc0 + src / np.maximum(occur, 1).astype(np.float32)[..., None]
    np.testing.assert_array_equal(_accumulate(src, occur, K, 1, h, w, acc0), want)
    # logits: the softmax of drs_tile_place_dihedral (one tile covering the whole map, g = 0) added into the same acc
    logits = (rng.normal(size=(1, h, w, K)) * 4).astype(np.float32)
    ref = torch.from_numpy(acc0.copy()).to(DEV)
    oc = torch.zeros(h * w, dtype=torch.int32, device=DEV)
    box = torch.tensor([[0, 0, 0, h, 0, w]], dtype=torch.int32, device=DEV)
    lg_dev = torch.from_numpy(logits).to(DEV)
    _lib.call("drs_tile_place_dihedral", ref.data_ptr(), oc.data_ptr(), lg_dev.data_ptr(), h, w, K, h, box.data_ptr(), 1, 0, stream())
    torch.cuda.synchronize()
    for occ in (np.ones((h, w)), np.zeros((h, w))):          # occur 0 counts as 1
        np.testing.assert_array_equal(_accumulate(logits[0], occ, K, 0, h, w, acc0), ref.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ against the oracle
H, W, BS = 160, 200, 4
NETS = {"dilated_grsl_rate8": 112, "dilated_icpr_rate6_densely": 72, "dilated_icpr_rate6_avgpool": 96}     # net: tile side
SCALES = (0.75, 1.25, 1.5)


@functools.lru_cache(maxsize=None)
def _oracle_scale(net_type, s, g=0):
    """U_s(softmax(F(g^-1 . g . Xs))): F = the fp64 oracle's whole-image eval forward of the resized, normalised image (transformed by
    the dihedral code g and mapped back), its probabilities resized back to H x W"""
    from drs_amd import patches as P
    _, o = _net(net_type, 2, 24, oracle=True)        # the same construction as the tests' nets
    hs, ws = P.scaled_size(H, s), P.scaled_size(W, s)
    x = _normalise(_torch_resample(_tile(H, W, seed=5), hs, ws)).astype(np.float64)
    lg = o.forward(np.ascontiguousarray(P.dihedral_apply(x, g))[None], False)[0]
    prob = np.ascontiguousarray(P.dihedral_apply(_softmax(lg), g, inverse=True))
    return _torch_resample(prob, H, W)


@pytest.mark.parametrize("net_type", sorted(NETS))
def test_every_scale_and_their_sum_match_the_oracle(net_type):
    from drs_amd import patches as P
    d, _ = _net(net_type, 2, 24)
    tile, T_ = _tile(H, W, seed=5), NETS[net_type]
    before, after = d.plan.receptive_field
    for s in SCALES:
        hs, ws = P.scaled_size(H, s), P.scaled_size(W, s)
        assert len(P.dense_tiles(hs, ws, T_, before, after)) > 2 * BS          # several tiles, several forwards, at every scale
        acc, occur, n = _dense(d, tile, BS, T_, (s,))
        assert (occur == 1).all() and n == len(P.dense_tiles(hs, ws, T_, before, after))
        assert rel_err(acc, _oracle_scale(net_type, s)) <= 1e-4, (net_type, s, rel_err(acc, _oracle_scale(net_type, s)))
    ref = sum(_oracle_scale(net_type, s) for s in SCALES)
    acc, occur, n = _dense(d, tile, BS, T_, SCALES)
    assert (occur == len(SCALES)).all()
    assert rel_err(acc, ref) <= 1e-4, (net_type, rel_err(acc, ref))
    pred, n2 = _dense(d, tile, BS, T_, SCALES, sums=False)
    assert n2 == n
    clear = _clear(ref)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(pred[clear], ref.argmax(-1)[clear])
    # the scales are not a no-op: the plain map is another function
    plain, _, _ = _dense(d, tile, BS, T_, (1.0,))
    assert rel_err(plain * len(SCALES), acc) > 1e-3


def test_scales_with_d4_match_the_oracle_mean_over_g():
    net_type, T_, scales = "dilated_icpr_rate6_densely", 72, (1.25, 0.75)
    d, _ = _net(net_type, 2, 24)
    acc, occur, _ = _dense(d, _tile(H, W, seed=5), BS, T_, scales, tta="d4")
    ref = sum(sum(_oracle_scale(net_type, s, g) for g in range(8)) / 8 for s in scales)
    assert (occur == 2).all()
    assert rel_err(acc, ref) <= 1e-4, rel_err(acc, ref)


# ------------------------------------------------------------------------------------------------------------ identities
def test_scale_one_is_the_single_scale_map_bitwise():
    d, _ = _net("dilated_grsl_rate8", 2, 24)
    tile = _tile(150, 230, seed=6)
    want, wocc, wn = _dense(d, tile, BS, 128, None, tta=(0,))
    for tta in ((0,), None):                  # logits placed and softmaxed on resampling, or softmax placed: the same bits
        acc, occur, n = _dense(d, tile, BS, 128, (1.0,), tta=tta)
        np.testing.assert_array_equal(acc, want)
        np.testing.assert_array_equal(occur, wocc)
        assert n == wn
    for group, g in (("flip", 4), ("d4", 8)):
        sums, socc, _ = _dense(d, tile, BS, 128, None, tta=group)
        acc, occur, _ = _dense(d, tile, BS, 128, (1.0,), tta=group)
        assert (socc == g).all() and (occur == 1).all()
        np.testing.assert_array_equal(acc, sums / np.float32(g))          # the division by 4 or 8 is exact
        np.testing.assert_array_equal(_dense(d, tile, BS, 128, (1.0,), tta=group, sums=False)[0],
                                      _dense(d, tile, BS, 128, None, tta=group, sums=False)[0])


def test_scales_map_does_not_depend_on_the_tile_side():
    d, _ = _net("dilated_grsl_rate8", 2, 24)
    tile = _tile(H, W, seed=7)
    a, _, _ = _dense(d, tile, BS, 112, (0.75, 1.25))
    b, _, _ = _dense(d, tile, BS, 150, (0.75, 1.25))
    assert rel_err(b, a) <= 1e-5, rel_err(b, a)
    again, _, _ = _dense(d, tile, BS, 150, (0.75, 1.25))
    np.testing.assert_array_equal(again, b)                       # deterministic: no float atomics


def test_one_twin_for_every_scale_and_smaller_tiles_on_a_larger_twin(monkeypatch):
    from drs_amd import loops, patches as P
    net_type = "dilated_grsl_rate8"
    d, _ = _net(net_type, 2, 24)
    made = []
    real = loops.DilatedNet

    def counting(*a, **kw):
        made.append(kw.get("s_max"))
        return real(*a, **kw)

    monkeypatch.setattr(loops, "DilatedNet", counting)
    _dense(d, _tile(H, W, seed=8), BS, 128, (0.75, 1.5, 1.0))      # T_s = 120, 128, 128
    assert made == [128] and d._dense_twin.s_max == 128
    monkeypatch.undo()
    # the logits of tiles of side T < s_max on the larger twin are those of a twin sized exactly T
    big = loops.dense_twin(d, 128, BS)
    pool = P.TilePool([_tile(H, W, seed=9)], None, DEV)
    inst = np.array([[0, 0, 0], [0, 30, 70], [0, 40, 60]])
    for T_, hs, ws in ((96, 240, 300), (80, 120, 150)):
        small = _net(net_type, 4, T_, seed=11)[0]                  # sized exactly T
        small.params.copy_(big.params)
        small.bn.copy_(big.bn)
        got, want = [], []
        for net, out in ((big, got), (small, want)):
            P.crop_resampled_to_net(net, pool, inst, T_, hs, ws, MEAN, STD, 5)
            out.append(net.forward(len(inst), T_, want_logits=True)[1].cpu().numpy())
        np.testing.assert_array_equal(got[0], want[0], err_msg="T=%d" % T_)


# ------------------------------------------------------------------------------------------------------------ data parallelism
def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import loops, patches as P
    from drs_amd.dist import TorchComm
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    d, _ = _net("dilated_grsl", 1, 24)
    pool = P.TilePool([_tile(160, 150, seed=12)], None, DEV)
    pred, n = loops.predict_tile_dense(d, pool, 0, 1, MEAN, STD, comm=comm, tile=80, scales=(0.75, 1.25))
    acc, occur, _ = loops.predict_tile_dense(d, pool, 0, 1, MEAN, STD, comm=comm, tile=80, scales=(0.75, 1.25), return_sums=True)
    facc, _, _ = loops.predict_tile_dense(d, pool, 0, 1, MEAN, STD, comm=comm, tile=80, scales=(1.25, 0.75), tta="flip",
                                          return_sums=True)
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out, pred=pred.cpu().numpy(), n=n, acc=acc.cpu().numpy(), occur=occur.cpu().numpy(), facc=facc.cpu().numpy())
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_scales_map_equals_single_rank():
    import tempfile
    from drs_amd import patches as P
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "scales_dp.npz")
        mp.spawn(_dp_worker, args=(2, 29400 + os.getpid() % 1000, out), nprocs=2, join=True)
        r = np.load(out)
        got, n, acc, occur, facc = r["pred"], int(r["n"]), r["acc"], r["occur"], r["facc"]
    d, _ = _net("dilated_grsl", 1, 24)
    tile = _tile(160, 150, seed=12)
    want, n1 = _dense(d, tile, 1, 80, (0.75, 1.25), sums=False)
    wacc, woccur, _ = _dense(d, tile, 1, 80, (0.75, 1.25))
    wfacc, _, _ = _dense(d, tile, 1, 80, (1.25, 0.75), tta="flip")
    before, after = d.plan.receptive_field
    assert len(P.dense_axis(120, 80, before, after)[0]) >= 3 and n == n1
    np.testing.assert_array_equal(got, want)     # one tile per forward on both sides: the same launches, bitwise
    np.testing.assert_array_equal(occur.reshape(160, 150), woccur)
    np.testing.assert_array_equal(acc.reshape(160, 150, K), wacc)
    np.testing.assert_array_equal(facc.reshape(160, 150, K), wfacc)


# ------------------------------------------------------------------------------------------------------------ the process surface
def test_scales_reject_se_nets_and_scales_too_small_for_the_margins():
    from drs_amd import loops, patches as P
    d, _ = _net("dilated_icpr_rate6_SE", 1, 24)
    pool = P.TilePool([_tile(64, 64, seed=9)], None, DEV)
    with pytest.raises(ValueError, match="squeeze-and-excitation"):
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=32, scales=(1.0, 1.5))
    d, _ = _net("dilated_grsl_rate8", 1, 24)
    pool = P.TilePool([_tile(160, 200, seed=10)], None, DEV)
    with pytest.raises(ValueError, match=r"scale 0\.5.*dilated_grsl_rate8"):          # 80 x 100 needs tiles of 80 <= 50 + 51
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, scales=(1.0, 0.5))
    with pytest.raises(ValueError, match=r"scale 1\.25.*dilated_grsl_rate8"):
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=100, scales=(1.25,))
    for bad in ((), (1.0, 1.0), (0.1,), (float("nan"),)):
        with pytest.raises(ValueError):
            loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=128, scales=bad)
    acc, occur, _ = loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, scales=(0.7,), return_sums=True)   # 112 x 140: one tile tall
    assert (occur == 1).all() and torch.isfinite(acc).all()


def test_validate_test_and_cli_dense_scales(tmp_path, monkeypatch, capsys):
    from drs_amd import cli, loops, patches as P
    from drs_amd.net import DilatedNet
    d, _ = _net("dilated_grsl_rate8", 2, 24)
    tile = _tile(140, 150, seed=13)
    lab = np.random.default_rng(2).integers(0, 7, size=(140, 150)).astype(np.uint8)
    want, _ = _dense(d, tile, 4, 128, (0.75, 1.25), tta="flip", sums=False)
    cm, maps = loops.validate_test(d, [tile], [lab], ["t0"], 4, MEAN, STD, 25, 0, dense_tile=128, dense_tta="flip",
                                   dense_scales=[0.75, 1.25])
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
    sc = cli.main(["--dense-scales=0.75,1.25"] + common + [out + "model-2"] + tail + ["generate_final_maps", "--dense-tile=128"],
                  device=DEV)
    text_sc = capsys.readouterr().out
    assert text_sc == text_plain and "--dense-" not in text_plain      # the flags are stripped before the parameters are printed
    np.testing.assert_array_equal(np.load(out + "top_mosaic_09cm_areac_class.npy"), sc[0])
    assert os.path.exists(out + "top_mosaic_09cm_areac_class.tif")
    net = DilatedNet("dilated8_grsl", CH, 6, 0.005, b_max=4, s_max=25, device=DEV)
    loops.load_checkpoint(net, out + "model-2")
    test_x, _ = cli.load_images("synthetic:140x150x5/vaihingen/", ["c"], "generate_final_maps")
    mean = np.load(os.path.join(str(tmp_path), "dataset_vaihingen_crop_25_stride_10_mean.npy"))
    std = np.load(os.path.join(str(tmp_path), "dataset_vaihingen_crop_25_stride_10_std.npy"))
    pool = P.TilePool(test_x, None, DEV)
    pd, _ = loops.predict_tile_dense(net, pool, 0, 4, mean, std, tile=128, scales=(0.75, 1.25))
    np.testing.assert_array_equal(sc[0], pd.cpu().numpy())
    pw, _ = loops.predict_tile(net, pool, 0, 25, 4, mean, std)
    np.testing.assert_array_equal(plain[0], pw.cpu().numpy())             # without the flags: the sliding windows, as before
    cm2, maps2 = cli.main(common + [out + "model-2"] + tail + ["validate_test", "--dense-tile=128", "--dense-scales=0.75,1.25",
                                                               "--dense-tta=d4"], device=DEV)
    pd4, _ = loops.predict_tile_dense(net, pool, 0, 4, mean, std, tile=128, scales=(0.75, 1.25), tta="d4")
    np.testing.assert_array_equal(maps2[0], pd4.cpu().numpy())
    with pytest.raises(SystemExit) as e:
        cli.main(common + [out + "model-2"] + tail + ["validate_test", "--dense-scales=0.75,1.25"], device=DEV)
    assert "--dense-tile" in str(e.value)
