"""CPU: the pieces of overlap-tile inference that need no GPU -- the library's receptive field of every net (against a count worked out
here from the oracle's tables), the tile plan (patches.dense_tiles) and the isprs command line's --dense-tile flag."""
import ctypes as C

import numpy as np
import pytest

from oracle import nets as N


def _block_field(spec, convs, i):
    """(before, after) one block adds: its conv's SAME pads, + 1 a side for the 3 x 3 max-pool, + a k x k average pool's SAME pads"""
    _, k, _, _, r = convs[i]
    b, a = N.same_pad(k, r)
    if spec["pool"]:
        b, a = b + 1, a + 1
    ak = spec.get("pools", [0] * len(convs))[i]
    if ak:
        pb, pa = N.same_pad(ak, 1)
        b, a = b + pb, a + pa
    return b, a


def _expected_field(net_type):
    """longest input-to-classifier path through the block graph of oracle/nets.py (the classifier is 1 x 1)"""
    spec = N.NETS[N.resolve(net_type)]
    convs = N.conv_specs(net_type, 5)
    f = [_block_field(spec, convs, i) for i in range(len(convs))]
    if spec.get("squeezes"):       # conv1, then per stage: squeeze -> (expand 1x1 | expand kxk) concatenated
        out = f[0]
        for i in range(1, len(convs), 3):
            s = (out[0] + f[i][0], out[1] + f[i][1])
            out = (s[0] + max(f[i + 1][0], f[i + 2][0]), s[1] + max(f[i + 1][1], f[i + 2][1]))
        return out
    if spec["dense"]:              # block i reads the concat of blocks 0..i-1 (block 0 the image); the classifier reads all of them
        reach = []
        for i in range(len(convs)):
            prev = [(0, 0)] if i == 0 else reach
            reach.append((f[i][0] + max(p[0] for p in prev), f[i][1] + max(p[1] for p in prev)))
        return max(p[0] for p in reach), max(p[1] for p in reach)
    return sum(v[0] for v in f), sum(v[1] for v in f)


def _library_field(net_type):
    from drs_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    _lib.call("drs_net_create", net_type.encode(), 5, 6, 0.0, 1, 1, 1, 0.5, C.byref(h))
    try:
        b, a = C.c_int(-1), C.c_int(-1)
        rc = lib.drs_net_receptive_field(h, C.byref(b), C.byref(a))
        return rc, (b.value, a.value)
    finally:
        lib.drs_net_destroy(h)


def test_receptive_field_of_every_net_matches_the_oracle_tables():
    from drs_amd import Plan, known_net_types
    for t in known_net_types():
        rc, got = _library_field(t)
        if N.NETS[N.resolve(t)].get("se"):
            assert rc == 1, t                       # DRS_ERR_ARG: a mean over the whole patch has no finite field
            assert Plan(t, 5, 6).receptive_field is None
            continue
        assert rc == 0, t
        assert got == _expected_field(t), (t, got)
        assert Plan(t, 5, 6).receptive_field == got
    assert _library_field("dilated_grsl_rate8")[1] == (50, 51)
    assert _library_field("dilated8_grsl")[1] == (50, 51)
    from drs_amd import _lib
    assert _lib.load().drs_net_receptive_field(None, None, None) == 1


def _check_plan(h, w, T, b, a):
    from drs_amd import patches as P
    boxes = P.dense_tiles(h, w, T, b, a)
    cover = np.zeros((h, w), dtype=np.int32)
    for y0, x0, cy0, cy1, cx0, cx1 in boxes:
        assert 0 <= y0 and y0 + T <= h and 0 <= x0 and x0 + T <= w          # the tile lies inside the image
        assert y0 <= cy0 < cy1 <= y0 + T and x0 <= cx0 < cx1 <= x0 + T        # a non-empty core inside its tile
        assert cy0 == 0 or cy0 - y0 >= b
        assert cy1 == h or y0 + T - cy1 >= a
        assert cx0 == 0 or cx0 - x0 >= b
        assert cx1 == w or x0 + T - cx1 >= a
        cover[cy0:cy1, cx0:cx1] += 1
    assert (cover == 1).all()                                                   # the cores partition the image
    # row-major: a grid of tile rows x tile columns
    ys, xs = sorted(set(boxes[:, 0])), sorted(set(boxes[:, 1]))
    assert len(boxes) == len(ys) * len(xs)
    np.testing.assert_array_equal(boxes[:, 0], np.repeat(ys, len(xs)))
    np.testing.assert_array_equal(boxes[:, 1], np.tile(xs, len(ys)))
    if T == h:
        assert ys == [0]
    if T == w:
        assert xs == [0]
    return boxes


def test_dense_tiles_partition_and_margins_over_random_cases():
    from drs_amd import patches as P
    rng = np.random.default_rng(11)
    checked = rejected = 0
    while checked < 2000:
        h, w = int(rng.integers(1, 160)), int(rng.integers(1, 160))
        b, a = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        T = int(rng.integers(1, min(h, w) + 1))
        if T < max(h, w) and T <= b + a:          # an axis of several tiles needs a core step of at least one pixel
            with pytest.raises(ValueError):
                P.dense_tiles(h, w, T, b, a)
            rejected += 1
            continue
        _check_plan(h, w, T, b, a)
        checked += 1
    assert checked >= 2000 and rejected > 50


def test_dense_tiles_edge_cases():
    from drs_amd import patches as P
    # T = the image side: one tile along that axis, whatever the margins
    assert P.dense_tiles(40, 40, 40, 50, 51).tolist() == [[0, 0, 0, 40, 0, 40]]
    boxes = _check_plan(40, 300, 40, 10, 12)
    assert set(boxes[:, 0]) == {0} and len(boxes) > 1
    # the issue's arithmetic: a 6000 x 6000 mosaic, Dilated8Pooling (50, 51), T = 512 -> 15 x 15 tiles with 411-pixel cores
    boxes = P.dense_tiles(6000, 6000, 512, 50, 51)
    assert len(boxes) == 225 and boxes[1, 4] == 461 and boxes[1, 5] - boxes[1, 4] == 411
    for bad in [(100, 100, 101, 0, 0), (100, 200, 150, 0, 0), (100, 100, 50, 25, 25), (100, 100, 50, 30, 30), (100, 100, 0, 1, 1),
                (100, 100, 50, -1, 2)]:
        with pytest.raises(ValueError):
            P.dense_tiles(*bad)
    _check_plan(100, 100, 51, 25, 25)          # T = before + after + 1: cores of one pixel's step
    _check_plan(1, 1, 1, 0, 0)


def test_cli_dense_tile_flag_parser():
    from drs_amd.cli import parse_dense_tile
    base = ["isprs_dilated_random.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a,b", "c", "0.01", "0.005", "4", "3", "25", "10",
            "dilated8_grsl", "multi_fixed", "9,13", "acc", "generate_final_maps"]
    got, tile = parse_dense_tile(base)
    assert got == base and got is not base and tile is None
    for pos in (1, 5, len(base)):
        for flag, want in (("--dense-tile", 0), ("--dense-tile=256", 256), ("--dense-tile=1", 1)):
            argv = base[:pos] + [flag] + base[pos:]
            got, tile = parse_dense_tile(argv)
            assert got == base and tile == want, (pos, flag)
    for bad in ("--dense-tile=", "--dense-tile=abc", "--dense-tile=0", "--dense-tile=-4", "--dense-tile=12.5", "--dense-tile=2x",
                "--dense-tile= 64"):
        with pytest.raises(ValueError):
            parse_dense_tile(base + [bad])
    with pytest.raises(ValueError):
        parse_dense_tile(base + ["--dense-tile", "--dense-tile=64"])
    # look-alikes are positional arguments, as before
    for other in ("--dense-tiles", "-dense-tile", "--dense"):
        got, tile = parse_dense_tile(base + [other])
        assert got == base + [other] and tile is None


def test_cli_rejects_the_flag_for_training_and_keeps_the_usage_text(capsys):
    from drs_amd import cli
    from drs_amd.net import NoComm
    with pytest.raises(SystemExit) as e:
        cli.main(["isprs_dilated_random.py", "too", "few"], device="cpu", comm=NoComm())
    assert str(e.value) == "Usage: isprs_dilated_random.py " + " ".join(cli.ISPRS_PARAMS)
    argv = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "none", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
            "single_fixed", "25", "acc", "training", "--dense-tile=64"]
    with pytest.raises(SystemExit) as e:
        cli.main(argv, device="cpu", comm=NoComm())
    assert "--dense-tile" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv[:-1] + ["--dense-tile=x"], device="cpu", comm=NoComm())
    assert "positive integer" in str(e.value)
