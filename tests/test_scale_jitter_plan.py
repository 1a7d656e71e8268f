"""CPU: the pieces of the training crop's scale jitter that need no GPU -- the numpy statement of the definition
(tests/scale_jitter_ref.py) held to scipy's map_coordinates, the centre rule, the scale draws and their random streams, the range
check and the three command lines' --scale-jitter flag."""
import math
import random

import numpy as np
import pytest
from scipy import ndimage

import scale_jitter_ref as R

SCALES = (0.5, 0.7071067811865476, 1.0, 1.25, 2.0)


class _Pool(object):
    """what the host geometry reads of a TilePool"""

    def __init__(self, sizes):
        self.h = [s[0] for s in sizes]
        self.w = [s[1] for s in sizes]


# ------------------------------------------------------------------------------------------------- the statement
@pytest.mark.parametrize("shape,S", [((23, 31), 7), ((40, 12), 8), ((17, 29), 8), ((9, 9), 7)])
def test_statement_matches_map_coordinates(shape, S):
    """The statement and scipy.ndimage.map_coordinates(order=1, mode="nearest") read the same four neighbours with the same weights
    ly, lx (the coordinate u - 0.5 handed to scipy is the statement's own, and `nearest` clamps it to [0, n - 1] as the statement
    does); they differ in how the four products are formed and summed: the statement is (1-ly)((1-lx) v00 + lx v01) + ly(...), scipy
    sum_k (wy wx)_k v_k.  Either way a term is a value times two weights in [0, 1], one of them 1 - l rounded (three roundings), and a
    term passes through at most three rounded additions: each result is within gamma_6 = 6 u / (1 - 6 u) of sum_k |w_k v_k| <= M,
    M the largest of the four neighbours' magnitudes, u = 2^-53.  The two differ by at most 2 gamma_6 M < 6.001 eps M, eps = 2^-52."""
    rng = np.random.default_rng(shape[0] * 100 + S)
    h, w = shape
    x = rng.normal(size=(h, w, 3)) * 3
    lab = rng.integers(0, 6, size=(h, w)).astype(np.uint8)
    eps = np.finfo(np.float64).eps
    for s in SCALES + (0.25, 4.0, 0.9):
        for r, c in ((0, 0), (h, w), (h // 3, w // 2)):
            geo = R.geometry(r, c, S, s, h, w)
            got, glab, valid = R.resample_geo(x, lab, S, geo)
            uy, vy, y0, y1, _, yl = R.axis(S, geo[1], geo[0], h)
            ux, vx, x0, x1, _, xl = R.axis(S, geo[2], geo[0], w)
            np.testing.assert_array_equal(valid, vy[:, None] & vx[None, :])
            coords = np.stack(np.meshgrid(uy - 0.5, ux - 0.5, indexing="ij"))
            M = np.maximum(np.maximum(np.abs(x[y0][:, x0]), np.abs(x[y0][:, x1])), np.maximum(np.abs(x[y1][:, x0]), np.abs(x[y1][:, x1])))
            for ch in range(3):
                want = ndimage.map_coordinates(x[:, :, ch], coords, order=1, mode="nearest")
                err = np.abs(got[:, :, ch] - want)[valid]
                assert np.all(err <= 6.001 * eps * M[:, :, ch][valid]), (shape, S, s, r, c, err.max())
            # the label is the source pixel that contains the centre; invalid pixels are 0 / 0
            want_lab = lab[np.minimum(np.floor(uy).astype(int).clip(0), h - 1)][:, np.minimum(np.floor(ux).astype(int).clip(0), w - 1)]
            np.testing.assert_array_equal(glab[valid], want_lab[valid])
            assert np.all(got[~valid] == 0) and np.all(glab[~valid] == 0)
            if 2 * (S / (2.0 * s)) <= min(h, w):
                assert valid.all()
    # the map smaller than the footprint: 40 x 12 at s = 0.5 with S = 8 has a footprint of 16 > 12 columns
    if shape == (40, 12):
        _, _, valid = R.resample(x, lab, 3, 2, S, 0.5)          # cx = 6, u = 6 + 2 (p - 3.5): -1, 1, ..., 11, 13
        assert not valid[:, 0].any() and not valid[:, S - 1].any() and valid[:, 1:S - 1].all()


@pytest.mark.parametrize("S", [7, 8, 25])
def test_scale_one_is_the_plain_crop_bit_for_bit(S):
    rng = np.random.default_rng(S)
    h, w = 41, 37
    x = rng.normal(size=(h, w, 5))
    lab = rng.integers(0, 6, size=(h, w)).astype(np.uint8)
    for r, c in ((0, 0), (h, w), (h - S, w - S), (5, 9), (h - S + 1, 3)):
        rr, cc = min(r, h - S), min(c, w - S)
        got, glab, valid = R.resample(x, lab, r, c, S, 1.0)
        assert valid.all()
        np.testing.assert_array_equal(got, x[rr:rr + S, cc:cc + S])
        np.testing.assert_array_equal(glab, lab[rr:rr + S, cc:cc + S])
        _, _, _, _, l, _ = R.axis(S, R.centre(rr, S, 1.0, h), 1.0, h)
        assert (l == 0).all()


def test_centre_rule_keeps_a_fitting_footprint_inside_its_map():
    from drs_amd import patches as P
    rng = np.random.default_rng(7)
    fits = overhangs = 0
    for _ in range(4000):
        S = int(rng.integers(1, 40))
        h, w = int(rng.integers(S, 200)), int(rng.integers(S, 200))
        s = float(np.exp(rng.uniform(math.log(P.SCALE_MIN), math.log(P.SCALE_MAX))))
        if rng.integers(0, 4) == 0:
            s = float(rng.choice([0.25, 0.5, 1.0, 2.0, 4.0, S / h, S / w]))
            s = min(max(s, P.SCALE_MIN), P.SCALE_MAX)
        r, c = int(rng.integers(0, h + 5)), int(rng.integers(0, w + 5))
        step, cy, cx = R.geometry(r, c, S, s, h, w)
        pool = _Pool([(h, w)])
        np.testing.assert_array_equal(P.scale_geometry(np.array([[0, r, c]]), pool, S, [s])[0], [step, cy, cx])     # host == statement
        assert step == 1.0 / s
        for n, cc in ((h, cy), (w, cx)):
            a = S / (2.0 * s)
            u, valid, _, _, _, _ = R.axis(S, cc, step, n)
            if 2.0 * a <= n:
                fits += 1
                assert a <= cc <= n - a
                assert valid.all() and u[0] >= 0.0 and u[-1] <= n          # every pixel centre of a fitting footprint is in the map
            else:
                overhangs += 1
                assert cc == n / 2.0                                       # centred: the overhang is the same on both sides
                np.testing.assert_array_equal(valid, valid[::-1])
    assert fits > 1000 and overhangs > 100
    # at scale 1 the centre is r + S / 2 of the shifted window: the clamp never moves it
    for S, n, r in ((7, 23, 0), (7, 23, 16), (8, 40, 32), (8, 8, 0)):
        assert P.jitter_centre(r, S, 1.0, n) == r + S / 2.0 == R.centre(r, S, 1.0, n)


# ------------------------------------------------------------------------------------------------- the draws
def _instances(B):
    return np.array([[b % 2, 3 * b, 2 * b, (37 * b) % 360] for b in range(B)])


def _states():
    return random.getstate(), np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


@pytest.mark.parametrize("noise", ["host", "device"])
def test_jitter_leaves_the_global_streams_and_the_other_tables_alone(noise):
    from drs_amd import patches as P
    inst = _instances(12)
    random.seed(5)
    np.random.seed(5)
    plain = P.draw_augmentation(inst, 9, 4, noise=noise)
    after_plain = _states()
    random.seed(5)
    np.random.seed(5)
    jit = P.draw_augmentation(inst, 9, 4, noise=noise, scale_jitter=(0.75, 1.25), jitter_key=(123, 4))
    assert _same_state(after_plain, _states())
    for name in ("rot_on", "rot", "noise_on", "flip"):
        np.testing.assert_array_equal(getattr(plain, name), getattr(jit, name))
    assert plain.seed == jit.seed and plain.index0 == jit.index0
    if noise == "host":
        np.testing.assert_array_equal(plain.noise, jit.noise)
    assert plain.scale is None and plain.geo is None and jit.geo is None
    assert jit.scale.shape == (12,) and jit.scale.dtype == np.float64
    assert np.all(jit.scale >= 0.75) and np.all(jit.scale <= 1.25) and len(set(jit.scale)) == 12


def test_same_run_seed_and_step_give_the_same_scales():
    from drs_amd import patches as P
    a = P.draw_scales(16, (0.5, 2.0), (99, 7))
    np.random.seed(1)
    np.random.random(5)
    random.random()
    np.testing.assert_array_equal(a, P.draw_scales(16, (0.5, 2.0), (99, 7)))          # a resumed run: same key, same scales
    assert not np.array_equal(a, P.draw_scales(16, (0.5, 2.0), (99, 8)))              # another step
    assert not np.array_equal(a, P.draw_scales(16, (0.5, 2.0), (98, 7)))              # another run
    np.testing.assert_array_equal(a[:5], P.draw_scales(5, (0.5, 2.0), (99, 7)))       # a patch's scale is its place's
    np.testing.assert_array_equal(P.draw_scales(6, (1, 1), (3, 1)), np.ones(6))       # (1, 1): exactly 1
    np.testing.assert_array_equal(P.draw_scales(6, (2, 2), (3, 1)), np.full(6, 2.0))
    # log-uniform: the logarithm is uniform on [ln lo, ln hi] -- its mean and spread over many draws
    z = np.log(P.draw_scales(20000, (0.25, 4.0), (1, 2))) / math.log(4.0)
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1 / math.sqrt(3)) < 0.02 and z.min() >= -1 and z.max() <= 1
    for bad in (None, (1,), (1, 2, 3), (-1, 2), (1, 2 ** 64)):
        with pytest.raises(ValueError):
            P.draw_scales(4, (0.5, 2.0), bad)
    assert P.jitter_run_seed((2 ** 31 - 1, 2 ** 31 - 2)) == ((2 ** 31 - 1) << 32 | (2 ** 31 - 2)) < 2 ** 63


def test_a_ranks_slice_of_the_global_draw_is_what_shard_slice_selects():
    from drs_amd import patches as P
    from drs_amd.dist import shard_slice
    inst = _instances(12)
    np.random.seed(2)
    aug = P.draw_augmentation(inst, 9, 4, noise="host", scale_jitter=(0.5, 2.0), jitter_key=(11, 3))
    pool = _Pool([(40, 50), (33, 29)])
    geo = P.scale_geometry(inst, pool, 9, aug.scale)
    seen = []
    for world in (1, 3, 4):
        for rank in range(world):
            sl = shard_slice(12, rank, world)
            mine = aug.shard(sl)
            np.testing.assert_array_equal(mine.scale, aug.scale[sl])
            np.testing.assert_array_equal(mine.scale, P.draw_scales(12, (0.5, 2.0), (11, 3))[sl])
            for name in ("rot_on", "rot", "noise_on", "flip", "noise"):
                np.testing.assert_array_equal(getattr(mine, name), getattr(aug, name)[sl])
            assert mine.seed == aug.seed and mine.index0 == sl.start and mine.geo is None
            np.testing.assert_array_equal(P.scale_geometry(inst[sl], pool, 9, mine.scale), geo[sl])
            if world == 4:
                seen.append(mine.scale)
    np.testing.assert_array_equal(np.concatenate(seen), aug.scale)
    plain = P.draw_augmentation(inst, 9, 4).shard(shard_slice(12, 1, 3))
    assert plain.scale is None and plain.geo is None


def test_sync_rng_returns_the_pair_without_moving_a_single_process_streams():
    from drs_amd import loops
    from drs_amd.net import NoComm
    random.seed(3)
    np.random.seed(4)
    before = _states()
    pair = loops.sync_rng(NoComm())
    assert _same_state(before, _states())
    assert pair == loops.sync_rng(NoComm())                               # the same point of the same run: the same run seed
    assert pair == (random.getrandbits(31), int(np.random.randint(0, 2 ** 31 - 1)))      # what rank 0 would have drawn

    class _World(object):
        rank, world, sync_rng = 0, 2, True

        @staticmethod
        def broadcast_object(v):
            return v
    random.seed(3)
    np.random.seed(4)
    got = loops.sync_rng(_World())
    assert got == pair                                                    # several ranks: the pair that is broadcast, as before
    r, n = random.Random(pair[0]), np.random.RandomState(pair[1])
    assert random.getstate() == r.getstate() and np.array_equal(np.random.get_state()[1], n.get_state()[1])


# ------------------------------------------------------------------------------------------------- check / parse / command lines
def test_check_and_parse_scale_jitter():
    from drs_amd import patches as P
    assert P.check_scale_jitter((0.75, 1.25)) == (0.75, 1.25)
    assert P.check_scale_jitter([1, 1]) == (1.0, 1.0)
    assert P.check_scale_jitter((0.25, 4)) == (0.25, 4.0)
    assert P.check_scale_jitter((np.float32(0.5), np.int64(2))) == (0.5, 2.0)
    assert all(type(v) is float for v in P.check_scale_jitter([1, np.float64(2)]))
    for bad in (None, 1.0, "0.75,1.25", (), (1,), (1, 1, 1), (1.25, 0.75), (0.2, 1), (1, 4.5), (float("nan"), 1), (1, float("inf")),
                (-1, 1), (0, 1), (True, 1), ("1", "2"), (None, 1)):
        with pytest.raises(ValueError):
            P.check_scale_jitter(bad)
    assert P.parse_scale_jitter("0.75,1.25") == (0.75, 1.25)
    assert P.parse_scale_jitter("1,1") == (1.0, 1.0)
    assert P.parse_scale_jitter("0.25,4") == (0.25, 4.0)
    for bad in ("", "1", "1,", ",1", "1,2,3", "a,b", "1;2", " 1,2", "1,2 ", "1, 2", "2,1", "0.1,1", "1,5", "nan,1", "1,inf", None):
        with pytest.raises(ValueError):
            P.parse_scale_jitter(bad)


def test_cli_flag_parser():
    from drs_amd import cli
    base = ["prog", "a", "b", "c"]
    got, j = cli.parse_scale_jitter(base)
    assert got == base and got is not base and j is None
    for pos in (1, 2, 4):
        got, j = cli.parse_scale_jitter(base[:pos] + ["--scale-jitter=0.75,1.25"] + base[pos:])
        assert got == base and j == (0.75, 1.25)
    for bad in ("--scale-jitter", "--scale-jitter=", "--scale-jitter=1", "--scale-jitter=2,1", "--scale-jitter=0.1,1", "--scale-jitter=1,2,3",
                "--scale-jitter=a,b", "--scale-jitter= 1,2", "--scale-jitter=1, 2"):
        with pytest.raises(ValueError) as e:
            cli.parse_scale_jitter(base + [bad])
        assert "--scale-jitter=lo,hi" in str(e.value) and "0.25" in str(e.value)
    with pytest.raises(ValueError, match="--scale-jitter given more than once"):
        cli.parse_scale_jitter(base + ["--scale-jitter=1,2", "--scale-jitter=1,2"])
    for other in ("--scale-jitte", "-scale-jitter", "--scale-jitter2"):
        assert cli.parse_scale_jitter(base + [other]) == (base + [other], None)
    # beside the other training options, in any order: each parser takes its own flag only
    argv = ["prog", "--focal-gamma=2", "p1", "--scale-jitter=0.5,2", "--class-weights=median", "p2"]
    argv, cw = cli.parse_class_weights(argv, 6)
    argv, g = cli.parse_focal_gamma(argv)
    argv, j = cli.parse_scale_jitter(argv)
    assert (argv, cw, g, j) == (["prog", "p1", "p2"], "median", 2.0, (0.5, 2.0))


def test_cli_mains_report_a_bad_flag_before_anything_else():
    from drs_amd import cli
    for main in (cli.main, cli.main_coffee, cli.main_contest):
        with pytest.raises(SystemExit) as e:
            main(["prog", "--scale-jitter=2,1"], device="cpu")
        assert "--scale-jitter=lo,hi" in str(e.value)
        with pytest.raises(SystemExit) as e:
            main(["prog", "--scale-jitter=1,2", "--scale-jitter=1,2"], device="cpu")
        assert "--scale-jitter given more than once" in str(e.value)
        with pytest.raises(SystemExit) as e:                      # a good flag is taken out before the positional arguments are counted
            main(["prog", "--scale-jitter=0.75,1.25"], device="cpu")
        assert str(e.value).startswith("Usage: ")


def test_cli_outside_training_is_refused():
    """isprs: the validate_test and generate_final_maps processes; contest: the test operation; coffee's command line has no process
    but training, so there the flag is always in place (the test above shows it parsed)."""
    from drs_amd import cli
    isprs = ["prog"] + ["x"] * 15
    for process in ("validate_test", "generate_final_maps"):
        with pytest.raises(SystemExit) as e:
            cli.main(isprs + [process, "--scale-jitter=0.75,1.25"], device="cpu")
        assert str(e.value) == "--scale-jitter applies to the training process only"
    contest = ["prog", "--scale-jitter=0.75,1.25"] + ["x"] * 13
    with pytest.raises(SystemExit) as e:
        cli.main_contest(contest + ["test"], device="cpu")
    assert "--scale-jitter applies to the train operation only" in str(e.value)


def test_train_loops_take_the_keyword_and_check_it_first():
    import inspect
    from drs_amd import loops, loops_indexed
    for fn in (loops.train, loops_indexed.train):
        p = inspect.signature(fn).parameters["scale_jitter"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    from drs_amd.net import NoComm
    said = []
    j, seed = loops.setup_scale_jitter([0.75, 1.25], (5, 6), NoComm(), said.append)
    assert j == (0.75, 1.25) and seed == (5 << 32 | 6)
    assert len(said) == 1 and said[0].startswith("Scale jitter: ") and "[0.75, 1.25]" in said[0]
    with pytest.raises(ValueError):
        loops.setup_scale_jitter((2, 1), (5, 6), NoComm(), said.append)
