"""CPU: the pieces of multi-scale test-time augmentation (loops.predict_tile_dense's scales) that need no GPU -- the scaled size, the
scale list check, the isprs command line's --dense-scales flag, the process-level checks and the numpy statement of the bilinear rule
(DESIGN.md 8a.2), held to torch's interpolate; the GPU tests use that statement as their oracle."""
import math

import numpy as np
import pytest
import torch


def resample_axis(n, ns):
    """one axis of D(n -> ns): (i0, i1, l) per output index, fp64 (include/drs.h)"""
    d = np.arange(ns, dtype=np.float64)
    src = np.maximum((d + 0.5) * (float(n) / float(ns)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, src - i0


def resample(x, hs, ws):
    """bilinear, half-pixel centres, on the first two axes of x (fp64): (1-ly)((1-lx) v00 + lx v01) + ly((1-lx) v10 + lx v11)"""
    x = np.asarray(x, dtype=np.float64)
    y0, y1, ly = resample_axis(x.shape[0], hs)
    x0, x1, lx = resample_axis(x.shape[1], ws)
    ly = ly.reshape((-1, 1) + (1,) * (x.ndim - 2))
    lx = lx.reshape((1, -1) + (1,) * (x.ndim - 2))
    r0, r1 = x[y0], x[y1]
    return (1 - ly) * ((1 - lx) * r0[:, x0] + lx * r0[:, x1]) + ly * ((1 - lx) * r1[:, x0] + lx * r1[:, x1])


def _torch_resample(x, hs, ws):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).permute(2, 0, 1)[None]
    out = torch.nn.functional.interpolate(t, size=(hs, ws), mode="bilinear", align_corners=False, antialias=False)
    return out[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("shape", [(37, 53), (160, 200), (5, 1), (1, 7)])
def test_bilinear_statement_matches_torch_interpolate(shape):
    from drs_amd import patches as P
    rng = np.random.default_rng(1)
    x = rng.normal(size=shape + (5,)) * 3
    h, w = shape
    # torch's CPU kernel rounds the source coordinate (d + 0.5) (n / ns) - 0.5 once (a fused multiply-add), the statement twice: the
    # weights may then differ by one ulp of the coordinate, so the bound is 1e-14 of the values plus that ulp times their spread
    tol = 1e-14 * np.abs(x).max() + np.spacing(float(max(h, w))) * np.ptp(x)
    for s in (0.25, 0.5, 0.75, 0.9, 1.0, 1.1, 1.25, 1.5, 2.0, 3.7):
        hs, ws = P.scaled_size(h, s), P.scaled_size(w, s)
        got, want = resample(x, hs, ws), _torch_resample(x, hs, ws)
        assert got.shape == want.shape == (hs, ws, 5)
        assert np.abs(got - want).max() <= tol, (shape, s, np.abs(got - want).max())
    for hs, ws in ((h + 3, w), (h, 2 * w + 1), (max(1, h - 2), max(1, w // 3))):       # unequal factors per axis
        assert np.abs(resample(x, hs, ws) - _torch_resample(x, hs, ws)).max() <= tol
    ident = resample(x, h, w)
    np.testing.assert_array_equal(ident, x)                  # ns = n: the identity, bit for bit
    i0, i1, lw = resample_axis(h, h)
    np.testing.assert_array_equal(i0, np.arange(h))
    assert (lw == 0).all()


def test_scaled_size():
    from drs_amd import patches as P
    assert P.scaled_size(6000, 0.75) == 4500 and P.scaled_size(6000, 1.25) == 7500 and P.scaled_size(6000, 1.0) == 6000
    assert P.scaled_size(5, 0.5) == 3              # 2.5 rounds half up
    assert P.scaled_size(3, 0.5) == 2 and P.scaled_size(7, 0.5) == 4
    assert P.scaled_size(1, 0.25) == 1 and P.scaled_size(2, 0.25) == 1 and P.scaled_size(3, 0.25) == 1    # never below 1
    assert P.scaled_size(160, 1.5) == 240 and P.scaled_size(200, 0.75) == 150
    for n in (1, 2, 17, 160, 6000):
        for s in (0.25, 0.6, 1.0, 1.3, 4.0):
            assert P.scaled_size(n, s) == max(1, math.floor(n * s + 0.5))
    assert isinstance(P.scaled_size(np.int64(10), np.float32(1.5)), int)


def test_check_scales():
    from drs_amd import patches as P
    assert P.check_scales([0.75, 1, 1.25]) == (0.75, 1.0, 1.25)
    assert P.check_scales((1.25, 0.75)) == (1.25, 0.75)            # the order given is kept: it is the order of the sum
    assert P.check_scales([0.25, 4]) == (0.25, 4.0)
    assert P.check_scales([np.float64(1.5), np.int64(2)]) == (1.5, 2.0)
    assert all(type(v) is float for v in P.check_scales([1, np.float32(0.5)]))
    for bad in ([], (), None, "1", 1.0, [float("nan")], [float("inf")], [1.0, -float("inf")], [0.2499], [4.01], [0], [-1],
                [1, 1.0], [0.5, 2, 0.5], [True], ["1"], [None]):
        with pytest.raises(ValueError):
            P.check_scales(bad)


BASE = ["isprs_dilated_random.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a,b", "c", "0.01", "0.005", "4", "3", "25", "10",
        "dilated8_grsl", "multi_fixed", "9,13", "acc", "generate_final_maps", "--dense-tile=64"]


def test_cli_dense_scales_flag_parser():
    from drs_amd.cli import parse_dense_scales, parse_dense_tile, parse_dense_tta
    got, scales = parse_dense_scales(BASE)
    assert got == BASE and got is not BASE and scales is None
    for pos in (1, 5, len(BASE)):
        got, scales = parse_dense_scales(BASE[:pos] + ["--dense-scales=0.75,1,1.25"] + BASE[pos:])
        assert got == BASE and scales == (0.75, 1.0, 1.25), pos
    assert parse_dense_scales(BASE + ["--dense-scales=1.5"])[1] == (1.5,)
    assert parse_dense_scales(BASE + ["--dense-scales=2,0.5"])[1] == (2.0, 0.5)
    for bad in ("--dense-scales", "--dense-scales=", "--dense-scales=0.75,,1", "--dense-scales=0.75;1", "--dense-scales=a",
                "--dense-scales= 1", "--dense-scales=1, 2", "--dense-scales=1,", "--dense-scales=nan", "--dense-scales=inf",
                "--dense-scales=0.1", "--dense-scales=5", "--dense-scales=1,1"):
        with pytest.raises(ValueError):
            parse_dense_scales(BASE + [bad])
    with pytest.raises(ValueError, match="more than once"):
        parse_dense_scales(BASE + ["--dense-scales=1", "--dense-scales=1"])
    for other in ("--dense-scale", "-dense-scales", "--dense-scales1", "--dense-t"):
        got, scales = parse_dense_scales(BASE + [other])
        assert got == BASE + [other] and scales is None
    # with the other two flags, in any order: each parser takes its own flag only
    argv = ["--dense-tta=d4"] + BASE[:3] + ["--dense-scales=1,0.5"] + BASE[3:]
    rest, tile = parse_dense_tile(argv)
    rest, tta = parse_dense_tta(rest)
    rest, scales = parse_dense_scales(rest)
    assert rest == BASE[:-1] and tile == 64 and tta == "d4" and scales == (1.0, 0.5)


def test_cli_rejects_dense_scales_without_dense_tile_and_bad_values():
    from drs_amd import cli
    from drs_amd.net import NoComm
    argv = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
            "single_fixed", "25", "acc", "generate_final_maps"]
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-scales=0.75,1"], device="cpu", comm=NoComm())
    assert "--dense-tile" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-scales=0.75,1", "--dense-tta=d4"], device="cpu", comm=NoComm())
    assert "--dense-tile" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-tile=64", "--dense-scales"], device="cpu", comm=NoComm())
    assert "--dense-scales=" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-tile=64", "--dense-scales=1", "--dense-scales=2"], device="cpu", comm=NoComm())
    assert "more than once" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-tile=64", "--dense-scales=0.1"], device="cpu", comm=NoComm())
    assert "0.25" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv[:-1] + ["training", "--dense-tile=64", "--dense-scales=1"], device="cpu", comm=NoComm())
    assert "--dense-tile applies" in str(e.value)


def test_loops_reject_scales_without_overlap_tiles():
    from drs_amd import loops
    with pytest.raises(ValueError, match="dense_tile"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, dense_scales=[0.75, 1])
    with pytest.raises(ValueError, match="dense_tile"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, dense_tta="d4", dense_scales=[0.75, 1])
    with pytest.raises(ValueError, match="dense_tile"):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, dense_scales=[1.5])
    with pytest.raises(ValueError):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, dense_tile=64, dense_scales=[])
    with pytest.raises(ValueError):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, dense_tile=64,
                                  dense_scales=[1, 1])


def test_config5_scaled_plans():
    """the tile counts behind DESIGN.md 8a.2's cost prediction: config 5 (6000^2, Dilated8Pooling margins 50 / 51, T = 512)"""
    from drs_amd import patches as P
    counts = {}
    for s in (0.75, 1.0, 1.25):
        n = P.scaled_size(6000, s)
        counts[s] = len(P.dense_tiles(n, n, min(n, 512), 50, 51))
    assert counts == {0.75: 121, 1.0: 225, 1.25: 361}
    assert abs(sum(counts.values()) / counts[1.0] - 707 / 225) < 1e-12          # 3.14: the expected cost against one scale
