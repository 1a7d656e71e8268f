"""-m gpu: the device-side noise of the training crop (noise="device": what the headline step feeds) against its counter-based
reference, tests/philox_ref.py -- Philox-4x32-10 + Box-Muller keyed by (seed, global element index before the flip), checked
against the published known answers in tests/test_philox_ref.py -- through drs_crop_normalize and drs_crop_normalize_scaled.

The kernel is a deterministic function of integers, so it is held to the reference element by element: the expected patch is the
NOISELESS crop, read back from the same entry point with noise_on = 0 and mean 0 / std 1, plus 0.01 x the reference deviate,
normalised as the kernel does it.  The maps hold multiples of 2^-12 in [0, 1) and the scales are 0.5 / 1 / 2 (bilinear weights are
multiples of 1/4, so an interpolated value is a multiple of 2^-16 below 1): every noiseless value is exact in float32, asserted below
on the fp64 statement of the scaled crop.  Device and numpy log / cos may differ in the last fp64 bit, which moves the stored float32
by at most one ulp, and that only where the fp64 value sits within ~1e-16 relative of a rounding boundary: a relative perturbation
of 4e-16 of the deviate flips none of 3072 roundings of values in [0, 1), so at most one element in 10 000 may differ at all.

The moment checks of test_gpu_patches.py / test_gpu_scale_jitter.py pass with the same deviate in every channel, the index taken
after the flip, the batch offset applied twice, the upper seed word ignored or a sigma wrong by 1.9 x; the negative controls at
the end show that these inputs tell such mistakes apart."""
import numpy as np
import pytest
import torch

import philox_ref as R
import scale_jitter_ref as J

pytestmark = pytest.mark.gpu

from gpu_util import DEV   # noqa: E402

SIZES = ((23, 31), (40, 12), (17, 29))
# (map, row, col, angle): top-left; the narrow map; bottom-right, where the shift-back applies (twice); interior
INST = np.array([[0, 0, 0, 30], [1, 10, 2, 45], [2, 17, 29, 90], [0, 9, 13, 45], [1, 40, 12, 315]])
B = len(INST)
NOISE_ON = np.array([1, 0, 1, 1, 1], dtype=np.uint8)
FLIP = np.array([0, 1, 2, 1, 2], dtype=np.int32)
ROTATED = 3                                     # this patch turns by 45 degrees: its corners are rotated-in fill, 0 + noise
SCALES = np.array([2.0, 0.5, 1.0, 1.0, 0.5])    # 0.5 on the narrow map: the footprint overhangs (invalid pixels: 0 + noise)
MEAN, STD = np.array([0.5, 0.4, 0.3, 0.0, 0.0]), np.array([0.25, 0.2, 0.1, 1.0, 1.0])
SEEDS = (12345, (7 << 32) | 12345)              # below 2^31, as draw_augmentation draws it; and one with an upper word (the ABI takes 64 bits)
SHARD = slice(2, 5)

_NETS = {}


def _net(C):
    from drs_amd.net import DilatedNet
    if C not in _NETS:
        _NETS[C] = DilatedNet("dilated_grsl", C, 6, 0.005, b_max=B, s_max=8, device=DEV)
    return _NETS[C]


def _maps(C):
    rng = np.random.default_rng(20 + C)
    tiles = [rng.integers(0, 4096, size=(h, w, C)).astype(np.float64) / 4096.0 for h, w in SIZES]
    labs = [rng.integers(0, 6, size=(h, w)).astype(np.uint8) for h, w in SIZES]
    return tiles, labs


def _crop(P, net, pool, inst, S, mean, std, aug):
    slab, Pd, ld = net.input_slab()
    slab.fill_(7.0)                      # a kernel that forgets the halo or the padded channels shows
    assert (Pd, ld) == (2, 8)
    P.crop_to_net(net, pool, inst, S, mean, std, aug)
    torch.cuda.synchronize()
    n, Sp = len(inst), S + 2 * Pd
    return slab[:n * Sp * Sp * ld].cpu().numpy().reshape(n, Sp, Sp, ld).copy()


def _aug(P, pool, S, seed, scaled, noise=True):
    aug = P.Augmentation(B)
    aug.flip[:] = FLIP
    if noise:
        aug.noise_on[:] = NOISE_ON
    aug.rot_on[ROTATED] = 1
    aug.rot[ROTATED] = P.rotation_params(INST[ROTATED, 3], S)
    aug.seed = seed
    if scaled:
        aug.scale, aug.geo = SCALES, P.scale_geometry(INST, pool, S, SCALES)
    return aug


def _shard(aug, sl):
    mine = aug.shard(sl)
    if aug.geo is not None:
        mine.geo = aug.geo[sl]
    return mine


def _indices(S, C, b_global, flips, pre_flip=True):
    """element index ((b * S + fi) * S + fj) * C + c of every output element [n][S][S][C]; (fi, fj) = the coordinates before the flip
    (pre_flip False: the output coordinates themselves -- a negative control)"""
    n = len(flips)
    i, j = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    idx = np.zeros((n, S, S, C), dtype=np.uint64)
    for q in range(n):
        fi = S - 1 - i if pre_flip and flips[q] == 1 else i
        fj = S - 1 - j if pre_flip and flips[q] == 2 else j
        idx[q] = (((int(b_global[q]) * S + fi) * S + fj)[:, :, None] * C + np.arange(C)).astype(np.uint64)
    return idx


def _ulp_report(got, want):
    """(elements that differ at all, elements further than one float32 ulp apart)"""
    got, want = got.astype(np.float32), want.astype(np.float32)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return int((got != want).sum()), int((diff > np.spacing(np.abs(want)).astype(np.float64)).sum())


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("C", [3, 5])
@pytest.mark.parametrize("S", [7, 8])
def test_device_noise_matches_the_counter_based_reference(S, C, f64):
    from drs_amd import patches as P
    tiles, labs = _maps(C)
    pool, net = P.TilePool(tiles, labs, DEV, dtype=np.float64 if f64 else np.float32), _net(C)
    for t in tiles:
        assert np.array_equal(t, t.astype(np.float32))
    for (m, r, c, _), s in zip(INST, SCALES):         # the scaled crop's noiseless values are exact in float32 (fp64 statement)
        img = J.resample(tiles[m], labs[m], r, c, S, s)[0]
        assert np.array_equal(img, img.astype(np.float32).astype(np.float64))
    mean, std, Pd = MEAN[:C], STD[:C], 2
    noisy = NOISE_ON.astype(bool)
    inner = (slice(None), slice(Pd, Pd + S), slice(Pd, Pd + S))
    worst = 0
    for scaled in (False, True):
        clean = _crop(P, net, pool, INST, S, np.zeros(C), np.ones(C), _aug(P, pool, S, 0, scaled, noise=False))     # the noiseless values
        base = _crop(P, net, pool, INST, S, mean, std, _aug(P, pool, S, 0, scaled, noise=False))                    # ... and normalised
        v = clean[inner][..., :C].astype(np.float64)
        assert (v[ROTATED, 0, 0] == 0).all() and (v[ROTATED, S // 2, S // 2] != 0).any()      # rotated-in fill in the corners
        for seed in SEEDS:
            aug = _aug(P, pool, S, seed, scaled)
            got = _crop(P, net, pool, INST, S, mean, std, aug)
            # 1. no noise where none was asked for: the other patches, the band-padding channels, the halo
            np.testing.assert_array_equal(got[~noisy], base[~noisy])
            np.testing.assert_array_equal(got[..., C:], base[..., C:])
            halo = got.copy()
            halo[inner] = base[inner]
            np.testing.assert_array_equal(halo, base)
            # 2. every noisy element against the reference
            idx = _indices(S, C, np.arange(B), FLIP)
            want = R.expected(v, seed, idx, mean, std)
            g = got[inner][..., :C]
            ndiff, nfar = _ulp_report(g[noisy], want[noisy])
            n = int(noisy.sum()) * S * S * C
            print("S %d C %d %s %s seed %#x: %d of %d elements differ, %d by more than one ulp" % (
                S, C, "f64" if f64 else "f32", "scaled" if scaled else "plain", seed, ndiff, n, nfar))
            worst = max(worst, ndiff)
            assert nfar == 0
            assert ndiff * 10000 <= n
            assert (g[noisy] != base[inner][..., :C][noisy]).mean() > 0.99          # (and the noise is there)
            # 3. a shard of the batch reproduces its rows of the whole batch, and so the reference at the GLOBAL patch index
            sub = _crop(P, net, pool, INST[SHARD], S, mean, std, _shard(aug, SHARD))
            np.testing.assert_array_equal(sub, got[SHARD])
            gs = sub[inner][..., :C]
            sd, sf = _ulp_report(gs[noisy[SHARD]], want[SHARD][noisy[SHARD]])
            assert sf == 0 and sd * 10000 <= gs[noisy[SHARD]].size
            # 4. negative controls, numpy only: each plausible mistake moves more than half of the noisy elements
            controls = {
                "index after the flip": (g, R.expected(v, seed, _indices(S, C, np.arange(B), FLIP, pre_flip=False), mean, std), noisy),
                "local batch index": (gs, R.expected(v[SHARD], seed, _indices(S, C, np.arange(3), FLIP[SHARD]), mean, std), noisy[SHARD]),
                "output words 2, 3": (g, R.expected(v, seed, idx, mean, std, words=(2, 3)), noisy),
            }
            if seed >> 32:
                controls["upper seed word dropped"] = (g, R.expected(v, seed & 0xffffffff, idx, mean, std), noisy)
            for name, (dev_out, wrong, sel) in controls.items():
                assert (dev_out[sel] != wrong[sel]).mean() > 0.5, name
    print("S %d C %d %s: at most %d differing elements in one call" % (S, C, "f64" if f64 else "f32", worst))
