"""CPU: the image-tile map of the plain forward / input-gradient launches (conv_mfma.hip, live_taps_image_tile in drs_common.hpp).

An M tile of the map holds the same Pc = 128 >> g columns of one image row of 2^g images, so a filter tap is dead for the whole tile
exactly when its shifted position leaves the image, in either axis.  Checked here without a GPU, through the development library:
the launch order the kernel reads from its table (a bijection, column tiles adjacent, every XCD chunk long tiles first and the same
K-step total to within one tile), the executed K-steps against a brute-force count, the shapes the map must refuse, and that the
row-tile order report (drs_debug_conv_order) is what it was.
"""
import ctypes as C

import numpy as np
import pytest

from drs_amd import _lib

# (B, S, k, rate, cin, cout, g)
SHAPES = [(128, 64, 3, 8, 256, 256, 7), (128, 64, 4, 3, 64, 128, 7), (128, 64, 5, 2, 64, 64, 7), (128, 64, 3, 5, 128, 192, 7),
          (256, 32, 3, 4, 128, 256, 7), (64, 64, 3, 6, 192, 192, 6), (32, 16, 3, 7, 64, 128, 5)]


def _pad_before(k, rate):
    return ((k - 1) * rate) // 2          # TensorFlow SAME, stride 1


def _bn(cout, cin):
    """N tile of the forward kernel (pick_conv_tile)"""
    if cout % 192 == 0 and cout % 128 != 0 and cin % 32 == 0:
        return 192
    return 128 if cout % 128 == 0 else (64 if cout % 64 == 0 else 32)


@pytest.fixture()
def lib():
    d = _lib.dev()
    old, old_sk = d.drs_debug_conv_image_tiles(-1), d.drs_debug_conv_splitk(-1)
    try:
        yield d
    finally:
        d.drs_debug_conv_image_tiles(old)
        d.drs_debug_conv_splitk(old_sk)


def _force(d, B, S, cout, g):
    """force 2^g images per tile; a launch of a few tiles would go stream-K by the cost model: keep it plain, as the GPU tests do"""
    d.drs_debug_conv_image_tiles(g)
    d.drs_debug_conv_splitk(0 if B * S * S // 128 < 1024 else -1)


def _order(d, fn, B, S, k, rate, pad, cin, cout):
    cap = 1 << 18
    out = np.full(cap, -1, dtype=np.int32)
    n = getattr(d, fn)(B, S, k, rate, pad, cin, cout, out.ctypes.data, cap)
    assert n <= cap
    return n, out[:max(n, 0)]


def _tile_taps(S, k, rate, pad, g):
    """brute force: live (tap row, tap column) pairs of the tile at (y, column group), [S][S / Pc]; a tile with none keeps all"""
    Pc = 128 >> g
    y = np.arange(S)
    liv_u = np.zeros(S, dtype=np.int64)
    liv_v = np.zeros(S // Pc, dtype=np.int64)
    for t in range(k):
        d = t * rate - pad
        liv_u += ((y + d >= 0) & (y + d < S))
        col_live = ((y + d >= 0) & (y + d < S)).reshape(S // Pc, Pc).any(axis=1)
        liv_v += col_live
    taps = liv_u[:, None] * liv_v[None, :]
    taps[taps == 0] = k * k
    return taps


def _executed(d, B, S, k, rate, pad, cin, cout):
    ex, tot = C.c_longlong(-1), C.c_longlong(-1)
    assert d.drs_conv_executed_ksteps(B, S, k, rate, pad, cin, cout, C.addressof(ex), C.addressof(tot)) == 0
    return ex.value, tot.value


@pytest.mark.parametrize("B,S,k,rate,cin,cout,g", SHAPES)
def test_order_is_a_balanced_long_first_bijection(lib, B, S, k, rate, cin, cout, g):
    pad = _pad_before(k, rate)
    _force(lib, B, S, cout, g)
    ntn = cout // _bn(cout, cin)
    mt = B * S * S // 128
    n, order = _order(lib, "drs_debug_conv_order_image", B, S, k, rate, pad, cin, cout)
    assert n == mt * ntn
    assert np.array_equal(np.sort(order), np.arange(n))                       # a bijection
    grp = order.reshape(mt, ntn)
    assert np.array_equal(grp, grp[:, :1] + np.arange(ntn)[None, :])          # the column tiles of an M tile are adjacent, in order
    assert np.all(grp[:, 0] % ntn == 0)
    # K-steps of every workgroup, from the brute-force tap count of its tile's position
    Pc = 128 >> g
    npc = S // Pc
    taps = _tile_taps(S, k, rate, pad, g)
    mtile = order // ntn
    ks = taps[(mtile // npc) % S, mtile % npc] * (cin // 32)
    assert n % 8 == 0
    chunks = ks.reshape(8, n // 8)                                            # xcd_remap: XCD c owns logical workgroups [c n/8, (c+1) n/8)
    assert np.all(np.diff(chunks, axis=1) <= 0)                               # long tiles first in every chunk
    tot = chunks.sum(axis=1)
    assert tot.max() - tot.min() <= ks.max() * ntn                            # the same total to within one (M) tile
    assert ks.min() < ks.max()                                                # (the shape does have short tiles)


@pytest.mark.parametrize("B,S,k,rate,cin,cout,g", SHAPES)
def test_executed_ksteps_match_brute_force(lib, B, S, k, rate, cin, cout, g):
    pad = _pad_before(k, rate)
    _force(lib, B, S, cout, g)
    ntn = cout // _bn(cout, cin)
    taps = _tile_taps(S, k, rate, pad, g)
    want = int(taps.sum()) * (B >> g) * ntn * (cin // 32)
    ex, tot = _executed(lib, B, S, k, rate, pad, cin, cout)
    assert tot == (B * S * S // 128) * ntn * k * k * (cin // 32)
    assert ex == want and ex < tot
    # pixel-level brute force of the same count at g = 7 (one position per tile): positions x taps whose shifted pixel is inside
    if g == 7:
        cnt = 0
        for y in range(S):
            for x in range(S):
                c = sum(1 for u in range(k) for v in range(k) if 0 <= y + u * rate - pad < S and 0 <= x + v * rate - pad < S)
                cnt += c if c else k * k
        assert ex == cnt * (B >> g) * ntn * (cin // 32)
    # with the map off the count is the row-tile rule's (whole tap rows only): never less than the image tiles'
    lib.drs_debug_conv_image_tiles(0)
    ex0, tot0 = _executed(lib, B, S, k, rate, pad, cin, cout)
    assert tot0 == tot and ex <= ex0 <= tot


REFUSED = [  # (B, S, k, rate, cin, cout, g, why)
    (48, 64, 3, 8, 256, 256, 5, "B is no multiple of 32"),
    (128, 10, 3, 2, 64, 128, 5, "S is no multiple of Pc = 4"),
    (18, 64, 3, 8, 256, 256, 4, "a stream-K launch"),
    (16, 40, 3, 8, 256, 256, 4, "a stream-K launch"),          # (B and S alone would allow g = 4 here)
    (128, 64, 1, 1, 256, 256, 7, "a single tap"),
    (128, 64, 5, 1, 8, 64, 7, "the few-band first layer is not on the LDS-DMA path"),
]


@pytest.mark.parametrize("B,S,k,rate,cin,cout,g,why", REFUSED)
def test_map_is_refused_and_the_order_stays(lib, B, S, k, rate, cin, cout, g, why):
    pad = _pad_before(k, rate)
    lib.drs_debug_conv_image_tiles(0)
    n0, before = _order(lib, "drs_debug_conv_order", B, S, k, rate, pad, cin, cout)
    ex0 = _executed(lib, B, S, k, rate, pad, cin, cout)
    lib.drs_debug_conv_image_tiles(g)
    n, _ = _order(lib, "drs_debug_conv_order_image", B, S, k, rate, pad, cin, cout)
    assert n == 0, why
    n1, after = _order(lib, "drs_debug_conv_order", B, S, k, rate, pad, cin, cout)
    assert n1 == n0 and np.array_equal(before, after)
    assert _executed(lib, B, S, k, rate, pad, cin, cout) == ex0
    if why == "a stream-K launch":
        assert lib.drs_debug_conv_sk_geometry((B * S * S // 128) * (cout // 128), k * k * (cin // 32), 128, None) > 0


def test_row_tile_order_report_is_unchanged(lib):
    """drs_debug_conv_order keeps describing the row-tile order whatever the image-tile switch says"""
    for (B, S, k, rate, cin, cout, g) in SHAPES:
        pad = _pad_before(k, rate)
        _force(lib, B, S, cout, 0)
        n0, a = _order(lib, "drs_debug_conv_order", B, S, k, rate, pad, cin, cout)
        _force(lib, B, S, cout, g)
        n1, b = _order(lib, "drs_debug_conv_order", B, S, k, rate, pad, cin, cout)
        assert n0 == n1 and np.array_equal(a, b)
    # the headline conv8 launch: 4096 M tiles x 2 column tiles, full tiles first (tests/test_wgrad_cut.py pins the details)
    lib.drs_debug_conv_image_tiles(7)
    n, o = _order(lib, "drs_debug_conv_order", 128, 64, 3, 8, 8, 256, 256)
    assert n == 8192 and np.array_equal(np.sort(o), np.arange(n))


def test_product_library_exports_the_query_only():
    p = _lib.load()
    assert hasattr(p, "drs_conv_executed_ksteps")
    assert not hasattr(p, "drs_debug_conv_image_tiles") and not hasattr(p, "drs_debug_conv_order_image")
    ex, tot = C.c_longlong(), C.c_longlong()
    assert p.drs_conv_executed_ksteps(128, 64, 3, 8, 8, 256, 256, C.addressof(ex), C.addressof(tot)) == 0
    assert 0 < ex.value <= tot.value == 4096 * 2 * 9 * 8
    assert p.drs_conv_executed_ksteps(128, 64, 3, 8, 8, 256, 256, None, None) != 0
