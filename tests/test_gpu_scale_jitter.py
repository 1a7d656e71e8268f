"""-m gpu: drs_crop_normalize_scaled -- the training crop with scale jitter -- against the numpy statement of its
definition (tests/scale_jitter_ref.py) composed with the host restatement of the reference's augmentation
(oracle.host_ref.dynamically_create_patches), bit for bit like the plain crop's tests; and loops.train with the option."""
import random
import re

import numpy as np
import pytest
import torch

import scale_jitter_ref as R
from oracle import host_ref as H

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

SIZES = ((23, 31), (40, 12), (17, 29))          # 40 x 12 is smaller than the footprint of a side-8 (and side-7) patch at s = 0.5
SCALES = np.array([0.7071067811865476, 0.5, 1.0, 1.25, 2.0])
# (map, row, col, angle): top-left; the narrow map (its columns overhang at 0.5); bottom-right, where the shift-back applies (twice);
# interior
INST = np.array([[0, 0, 0, 30], [1, 10, 2, 45], [2, 17, 29, 90], [0, 9, 13, 200], [1, 40, 12, 315]])
B = len(INST)
MEAN, STD = np.array([0.5, 0.4, 0.3, 0.0, 0.0]), np.array([0.25, 0.2, 0.1, 1.0, 1.0])


def _maps(C, f64):
    """three maps of different, non-square sizes (distinct tile_off / lab_off) as the pool holds them, taken to fp64"""
    rng = np.random.default_rng(10 + C)
    tiles = [rng.uniform(size=(h, w, C)) for h, w in SIZES]
    labs = [rng.integers(0, 6, size=(h, w)).astype(np.uint8) for h, w in SIZES]
    if not f64:
        tiles = [t.astype(np.float32).astype(np.float64) for t in tiles]
    return tiles, labs


_NETS = {}


def _net(C):
    from drs_amd.net import DilatedNet
    if C not in _NETS:
        _NETS[C] = DilatedNet("dilated_grsl", C, 6, 0.005, b_max=B, s_max=8, device=DEV)
    return _NETS[C]


def _pool(tiles, labs, f64):
    from drs_amd import patches as P
    return P.TilePool(tiles, labs, DEV, dtype=np.float64 if f64 else np.float32)


def _prefill(net):
    slab, Pd, ld = net.input_slab()
    slab.fill_(7.0)                      # a kernel that forgets the halo or the padded channels shows
    net.labels.fill_(255)
    net.acc_mask.fill_(255)
    assert (Pd, ld) == (2, 8)


def _read(net, n, S):
    slab, Pd, ld = net.input_slab()
    torch.cuda.synchronize()
    Sp = S + 2 * Pd
    a = slab[:n * Sp * Sp * ld].cpu().numpy().reshape(n, Sp, Sp, ld)
    M = n * S * S
    return a, net.labels[:M].cpu().numpy().reshape(n, S, S), net.acc_mask[:M].cpu().numpy().reshape(n, S, S)


def _resampled(tiles, labs, S, scales, inst=INST):
    """every patch's resampled S x S image, its labels and validity by the statement; validity is carried through the restatement in the
    label map: label + 1 where valid, 0 where not (0 is also what the rotation fills with)"""
    out = [R.resample(tiles[m], labs[m], r, c, S, s) for (m, r, c, _), s in zip(inst, scales)]
    return [o[0] for o in out], [np.where(o[2], o[1].astype(np.int64) + 1, 0).astype(np.uint8) for o in out]


def _slab_of(x, S, Pd=2, ld=8):
    """[n][S][S][C] float32 -> the haloed, channel-padded slab"""
    a = np.zeros((x.shape[0], S + 2 * Pd, S + 2 * Pd, ld), dtype=np.float32)
    a[:, Pd:Pd + S, Pd:Pd + S, :x.shape[3]] = x
    return a


def _geo(pool, S, scales, inst=INST):
    from drs_amd import patches as P
    return P.scale_geometry(inst, pool, S, scales)


# ------------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("C", [3, 5])
@pytest.mark.parametrize("S", [7, 8])
def test_scaled_crop_matches_the_statement_composed_with_the_reference_augmentation(S, C, f64):
    from drs_amd import patches as P
    tiles, labs = _maps(C, f64)
    pool, net = _pool(tiles, labs, f64), _net(C)
    patches, enc = _resampled(tiles, labs, S, SCALES)
    one = [[b, 0, 0, INST[b, 3]] for b in range(B)]              # each resampled patch is its own one-patch map
    for train in (True, False):
        if train:
            np.random.seed(77 + S)
            aug = P.draw_augmentation(INST, S, C, noise="host")
            assert aug.rot_on.any() and aug.noise_on.any() and len(set(aug.flip)) > 1
            np.random.seed(77 + S)
        else:
            aug = P.Augmentation(B)
        aug.scale, aug.geo = SCALES, _geo(pool, S, SCALES)
        x, lab1, rot_valid = H.dynamically_create_patches(patches, enc, one, S, is_train=train)
        valid = lab1 > 0
        assert not (valid & ~rot_valid).any()
        H.normalize_images(x, MEAN, STD)
        _prefill(net)
        P.crop_to_net(net, pool, INST, S, MEAN[:C], STD[:C], aug)
        a, lab, mask = _read(net, B, S)
        np.testing.assert_array_equal(a, _slab_of(x.astype(np.float32), S))          # interior, halo and padded channels
        np.testing.assert_array_equal(lab, np.where(valid, lab1 - 1, 0))
        np.testing.assert_array_equal(mask, valid.astype(np.uint8))
        if not train:                                             # the fitting footprints are whole; the narrow map's overhang is masked
            assert mask[[0, 2, 3, 4]].all()                       # (side 8: u = 6 + 2 (p - 3.5) = -1, 1, ..., 11, 13 on 12 columns;
            if S == 8:                                            #  side 7: u = 0, 2, ..., 12, the outermost centres on the map's edge)
                assert not mask[1][:, 0].any() and not mask[1][:, 7].any() and mask[1][:, 1:7].all()
            else:
                assert mask[1].all()


# ------------------------------------------------------------------------------------------------- 2. scale 1 is the plain crop
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("S,C", [(7, 5), (8, 3)])
def test_scale_one_equals_the_plain_entry_point(S, C, f64):
    from drs_amd import patches as P
    tiles, labs = _maps(C, f64)
    pool, net = _pool(tiles, labs, f64), _net(C)
    np.random.seed(5)
    aug = P.draw_augmentation(INST, S, C, noise="device")
    aug.rot_on[:2], aug.noise_on[1:3] = 1, 1
    for b in range(B):
        aug.rot[b] = P.rotation_params(INST[b, 3], S)
    _prefill(net)
    P.crop_to_net(net, pool, INST, S, MEAN[:C], STD[:C], aug, void_label=2)
    want = _read(net, B, S)
    aug.scale = np.ones(B)
    aug.geo = _geo(pool, S, aug.scale)
    _prefill(net)
    P.crop_to_net(net, pool, INST, S, MEAN[:C], STD[:C], aug, void_label=2)
    got = _read(net, B, S)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert want[2].any() and not want[2].all()


# ------------------------------------------------------------------------------------------------- 3. device noise by global index
@pytest.mark.parametrize("S,C,f64", [(7, 3, True), (8, 5, False)])
def test_device_noise_is_keyed_by_the_global_patch_index(S, C, f64):
    from drs_amd import patches as P
    tiles, labs = _maps(C, f64)
    pool, net = _pool(tiles, labs, f64), _net(C)
    aug = P.Augmentation(B)
    aug.noise_on[:] = 1
    aug.flip[:] = [0, 1, 2, 1, 2]
    aug.seed = 4242
    aug.scale, aug.geo = SCALES, _geo(pool, S, SCALES)
    _prefill(net)
    P.crop_to_net(net, pool, INST, S, MEAN[:C], STD[:C], aug)
    whole = _read(net, B, S)
    sl = slice(2, 5)
    mine = aug.shard(sl)
    assert mine.index0 == 2
    mine.geo = aug.geo[sl]
    _prefill(net)
    P.crop_to_net(net, pool, INST[sl], S, MEAN[:C], STD[:C], mine)
    part = _read(net, 3, S)
    for p, w in zip(part, whole):
        np.testing.assert_array_equal(p, w[sl])
    # and the noise is there: N(0, 0.01) on top of the noiseless crop
    aug.noise_on[:] = 0
    P.crop_to_net(net, pool, INST, S, [0, 0, 0], [1, 1, 1], aug)
    clean = _read(net, B, S)[0]
    aug.noise_on[:] = 1
    P.crop_to_net(net, pool, INST, S, [0, 0, 0], [1, 1, 1], aug)
    d = (_read(net, B, S)[0] - clean)[:, 2:2 + S, 2:2 + S, :C]
    assert 0.005 < d.std() < 0.02 and abs(d.mean()) < 0.005


# ------------------------------------------------------------------------------------------------- 4. float16 and the void label
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("S,C,f64", [(7, 3, False), (8, 3, True), (8, 5, False)])
def test_float16_modes_and_void_label_as_the_indexed_loops_feed_them(S, C, f64, mode):
    """loops_indexed.train's inputs: flips by index and no other augmentation, coffee's float16 pass (the resampled fp64 value rounded to
    float32, as coffee's patches are, then to float16; difference and quotient each rounded to float16 in the statistics' type) and
    contest's void label"""
    from drs_amd import patches as P
    tiles, labs = _maps(C, f64)
    pool, net = _pool(tiles, labs, f64), _net(C)
    void = 3
    flips = np.array([0, 1, 2, 2, 1], dtype=np.int32)
    patches, enc = _resampled(tiles, labs, S, SCALES)
    flip = {0: lambda z: z, 1: np.flipud, 2: np.fliplr}
    x16 = np.stack([flip[f](p) for f, p in zip(flips, patches)]).astype(np.float32).astype(np.float16)
    lab1 = np.stack([flip[f](e) for f, e in zip(flips, enc)])
    rng = np.random.default_rng(3)
    mean = (0.4 + 0.2 * rng.uniform(size=3)).astype(np.float32 if mode == 1 else np.float64)
    std = (0.1 + 0.2 * rng.uniform(size=3)).astype(mean.dtype)
    if mode == 1:
        want = H.normalize_images_f16(x16, mean, std)
    else:
        want = x16.copy()
        for c in range(3):                                        # coffee:67-74 with float64 scalars, by NumPy itself
            want[..., c] = np.subtract(want[..., c], mean[c])
            want[..., c] = np.divide(want[..., c], std[c])
    assert want.dtype == np.float16
    aug = P.Augmentation(B)
    aug.flip = flips
    aug.scale, aug.geo = SCALES, _geo(pool, S, SCALES)
    _prefill(net)
    P.crop_to_net(net, pool, INST, S, mean, std, aug, void_label=void, quantize_f16=True)
    a, lab, mask = _read(net, B, S)
    valid = lab1 > 0
    labels = np.where(valid, lab1.astype(np.int64) - 1, 0)
    np.testing.assert_array_equal(a, _slab_of(want.astype(np.float32), S))
    np.testing.assert_array_equal(lab, labels)
    np.testing.assert_array_equal(mask, (valid & (labels != void)).astype(np.uint8))
    assert (labels[valid] == void).any() and (S == 7 or not valid.all())


# ------------------------------------------------------------------------------------------------- 5. the device-side check
def test_a_bad_geo_row_or_map_index_zeroes_that_patch_only():
    """an argument check answered by the kernel's own guard: step = 0, a NaN step, an infinite centre, a map index past the pool and a
    negative one each leave a zero patch with labels 0 and mask 0; the patches beside them are what they are in a good batch"""
    from drs_amd import _lib, patches as P
    S, C = 8, 5
    tiles, labs = _maps(C, True)
    pool, net = _pool(tiles, labs, True), _net(C)
    aug = P.Augmentation(B)
    aug.noise_on[:] = 1
    aug.seed = 99
    aug.scale, aug.geo = SCALES, _geo(pool, S, SCALES)
    _prefill(net)
    P.crop_to_net(net, pool, INST, S, MEAN, STD, aug)
    good = _read(net, B, S)
    n = 7
    src = [0, 1, 2, 3, 4, 0, 1]
    inst = np.zeros((n, 4), dtype=np.int32)
    inst[:, 0] = INST[src, 0]
    geo = aug.geo[src].copy()
    geo[1, 0] = 0.0
    geo[3, 0] = np.nan
    geo[4, 2] = np.inf
    inst[5, 0], inst[6, 0] = len(SIZES), -1
    bad = [1, 3, 4, 5, 6]
    from drs_amd.net import DilatedNet
    big = DilatedNet("dilated_grsl", C, 6, 0.005, b_max=n, s_max=S, device=DEV)
    _prefill(big)
    slab, Pd, ld = big.input_slab()
    d_inst, d_geo, d_non = dev(inst), dev(geo), dev(np.ones(n, dtype=np.uint8))
    import ctypes
    m3, s3 = (ctypes.c_double * 3)(*MEAN[:3]), (ctypes.c_double * 3)(*STD[:3])
    _lib.call("drs_crop_normalize_scaled", pool.tiles.data_ptr(), 1, pool.labels.data_ptr(), pool.tile_off.data_ptr(),
              pool.lab_off.data_ptr(), pool.tile_h.data_ptr(), pool.tile_w.data_ptr(), len(SIZES), C, d_inst.data_ptr(), d_geo.data_ptr(),
              None, None, None, d_non.data_ptr(), 99, 0, ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), n, S, Pd, ld,
              slab.data_ptr(), big.labels.data_ptr(), big.acc_mask.data_ptr(), -1, 0, stream())
    a, lab, mask = _read(big, n, S)
    for b in bad:
        assert not a[b].any() and not lab[b].any() and not mask[b].any(), b
    for b in (0, 2):                                  # same place in the batch: same device noise
        np.testing.assert_array_equal(a[b], good[0][b])
        np.testing.assert_array_equal(lab[b], good[1][b])
        np.testing.assert_array_equal(mask[b], good[2][b])
    with pytest.raises(_lib.DrsError):                # host-side checks: no geo, no maps
        _lib.call("drs_crop_normalize_scaled", pool.tiles.data_ptr(), 1, pool.labels.data_ptr(), pool.tile_off.data_ptr(),
                  pool.lab_off.data_ptr(), pool.tile_h.data_ptr(), pool.tile_w.data_ptr(), len(SIZES), C, d_inst.data_ptr(), None,
                  None, None, None, d_non.data_ptr(), 99, 0, ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), n, S, Pd,
                  ld, slab.data_ptr(), big.labels.data_ptr(), big.acc_mask.data_ptr(), -1, 0, stream())
    with pytest.raises(_lib.DrsError):
        _lib.call("drs_crop_normalize_scaled", pool.tiles.data_ptr(), 1, pool.labels.data_ptr(), pool.tile_off.data_ptr(),
                  pool.lab_off.data_ptr(), pool.tile_h.data_ptr(), pool.tile_w.data_ptr(), 0, C, d_inst.data_ptr(), d_geo.data_ptr(),
                  None, None, None, d_non.data_ptr(), 99, 0, ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), n, S, Pd,
                  ld, slab.data_ptr(), big.labels.data_ptr(), big.acc_mask.data_ptr(), -1, 0, stream())
    with pytest.raises(ValueError):                   # crop_to_net: a geo table of the wrong shape
        aug.geo = aug.geo[:3]
        P.crop_to_net(net, pool, INST, S, MEAN, STD, aug)


# ------------------------------------------------------------------------------------------------- 6. the training loop
def test_train_loop_with_scale_jitter(tmp_path, capsys, monkeypatch):
    from drs_amd import loops, patches as P, sampling as SP
    from drs_amd.cli import init_size_scores
    from drs_amd.synthetic import make_tile
    t = [make_tile(64, 72, 5, 6, seed=1, n_seeds=20), make_tile(60, 66, 5, 6, seed=2, n_seeds=20)]
    data, labels = [t[0][0], t[1][0]], [t[0][1], t[1][1]]
    random.seed(0)
    np.random.seed(0)
    dist = SP.create_distributions_over_classes(labels, 25, 10)
    rot = SP.create_rotation_distribution(dist)
    mean, std = SP.dynamically_calculate_mean_and_std(data, dist, 25)
    values = [9, 13]
    real_crop = P.crop_to_net
    monkeypatch.setattr(loops, "SUPER_BATCH", 3)                   # 12 instances per super batch: the closing validation stays short

    def run(tag, jitter):
        seen = dict(rows=[], scaled=[], slab=None)

        def crop(net, pool, instances, S, mean_, std_, aug=None, **kw):
            out = real_crop(net, pool, instances, S, mean_, std_, aug, **kw)
            if aug is not None:                                  # a training crop (validation passes none)
                seen["rows"].append(np.array(instances))
                seen["scaled"].append(aug.geo is not None)
                if seen["slab"] is None:
                    slab, Pd, ld = net.input_slab()
                    seen["slab"] = slab[:len(instances) * (S + 2 * Pd) ** 2 * ld].cpu().numpy().copy()
            return out
        monkeypatch.setattr(P, "crop_to_net", crop)
        cache = tmp_path / tag
        cache.mkdir()
        random.seed(11)
        np.random.seed(11)
        acc, occ, chosen, probs = init_size_scores("multi_fixed", values)
        net = loops.train(data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 4, 3, 0.005, mean, std, "acc", "multi_fixed",
                          values, acc, occ, chosen, probs, 20, str(cache) + "/", 1, "dilated_grsl", "vaihingen", "none", device=DEV,
                          val_cache_dir=str(cache), scale_jitter=jitter)
        monkeypatch.setattr(P, "crop_to_net", real_crop)
        text = capsys.readouterr().out
        return net.state_dict(), seen, text

    plain, seen0, text0 = run("plain", None)
    jit, seen1, text1 = run("jitter", (0.75, 1.25))
    unit, seen2, text2 = run("unit", (1, 1))
    sizes = lambda text: [l for l in text.splitlines() if l.strip().isdigit()]                # noqa: E731
    assert len(sizes(text0)) >= 3 and sizes(text0) == sizes(text1) == sizes(text2)            # the size log lines
    for a, b, c in zip(seen0["rows"], seen1["rows"], seen2["rows"]):                         # ... and the instances
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    assert len(seen0["rows"]) == len(seen1["rows"]) == 3
    assert seen0["scaled"] == [False] * 3 and seen1["scaled"] == [True] * 3 and seen2["scaled"] == [True] * 3
    assert "Scale jitter" not in text0 and text1.count("Scale jitter: ") == 1 and "[0.75, 1.25]" in text1
    losses = [float(v) for v in re.findall(r"Training Minibatch: Loss= ([-+0-9.einfa]+)", text1)]
    assert len(losses) == 3 and np.all(np.isfinite(losses))
    assert seen0["slab"].shape == seen1["slab"].shape and not np.array_equal(seen0["slab"], seen1["slab"])      # the option reaches the kernel
    np.testing.assert_array_equal(seen0["slab"], seen2["slab"])
    assert sorted(plain) == sorted(unit)
    for k in plain:                                                # (1, 1): the plain run, bit for bit
        np.testing.assert_array_equal(np.asarray(plain[k]), np.asarray(unit[k]), err_msg=k)
    assert any(not np.array_equal(np.asarray(plain[k]), np.asarray(jit[k])) for k in plain)
