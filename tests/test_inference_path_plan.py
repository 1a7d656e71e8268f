"""No GPU: loops.InferencePath -- the one description of a whole-map inference path that validate_test, generate_final_maps and
fit_temperature dispatch through -- and cli._take_flag, the one optional-flag parser under every cli.parse_*."""
import pytest

from drs_amd import cli, loops
from drs_amd.loops import InferencePath


# the inputs test_dense_tta_plan, test_dense_scales_plan, test_dense_se_plan and test_temperature_plan give validate_test(None, [], ...)
@pytest.mark.parametrize("kw, say", [
    (dict(dense_tta="d4"), "test-time augmentation needs overlap-tile inference (dense_tile): the sliding-window map depends on the "
                           "patch size and has no exact dihedral form"),
    (dict(dense_tta="flip"), "test-time augmentation needs overlap-tile inference (dense_tile)"),
    (dict(dense_scales=[0.75, 1]), "multi-scale test-time augmentation needs overlap-tile inference (dense_tile): the sliding windows take "
                                   "their scales from the patch size (crop_sizes)"),
    (dict(dense_tta="d4", dense_scales=[0.75, 1]), "test-time augmentation needs overlap-tile inference (dense_tile)"),      # tta speaks first
    (dict(dense_scales=[1.5]), "multi-scale test-time augmentation needs overlap-tile inference (dense_tile)"),
    (dict(dense_se="global"), "whole-image squeeze-and-excitation gates need overlap-tile inference (dense_tile): a sliding window is "
                              "gated by its own mean"),
    (dict(dense_tile=64, dense_se="local"), "dense_se must be one of ['global'], not 'local'"),
    (dict(dense_tile=64, crop_sizes=[25, 18]), "overlap-tile inference has one scale: its map does not depend on a patch size"),
    (dict(dense_tile=0, dense_tta="d4", crop_sizes=[25]), "overlap-tile inference has one scale"),
])
def test_check_raises_the_messages_the_callers_raised(kw, say):
    with pytest.raises(ValueError) as e:
        InferencePath(crop_size=25, **kw).check()
    assert say in str(e.value)
    with pytest.raises(ValueError) as e2:                  # and the callers raise them through it, before they touch the net
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, **kw)
    assert str(e2.value) == str(e.value)
    with pytest.raises(ValueError) as e3:
        loops.fit_temperature(None, [], [], 1, None, None, 25, **kw)
    assert str(e3.value) == str(e.value)


@pytest.mark.parametrize("kw", [dict(dense_tile=64, dense_tta="rot"), dict(dense_tile=64, dense_scales=[]),
                                dict(dense_tile=64, dense_scales=[1, 1]), dict(dense_tile=64, dense_tta=(0, 9))])
def test_check_refuses_malformed_options_of_the_dense_path(kw):
    with pytest.raises(ValueError):
        InferencePath(crop_size=25, **kw).check()


def test_check_passes_what_goes_together_and_the_description_is_immutable():
    for kw in (dict(), dict(crop_sizes=[25, 18]), dict(flavour="contest"), dict(dense_tile=0), dict(dense_tile=96, dense_tta="d4"),
               dict(dense_tile=96, dense_scales=(0.75, 1.25), dense_tta="flip", dense_se="global")):
        assert InferencePath(crop_size=25, **kw).check() is None
    p = InferencePath(crop_size=25)
    assert p == (25, None, "isprs", None, None, None, None)
    with pytest.raises(AttributeError):
        p.dense_tile = 64
    assert p._replace(dense_tile=64).dense_tile == 64 and p.dense_tile is None


# DESIGN.md 8a.4, "Which path is in which mode"
@pytest.mark.parametrize("kind, kw, is_prob", [
    ("predict_tile", dict(), False),
    ("_predict_tile_bands", dict(flavour="isprs"), False),          # the same description: the bands are chosen by the number of ranks
    ("predict_tile_multiscale", dict(crop_sizes=[25, 33]), True),
    ("predict_tile_dense", dict(dense_tile=0), False),
    ("predict_tile_dense + tta", dict(dense_tile=96, dense_tta="flip"), True),
    ("predict_tile_dense + scales", dict(dense_tile=96, dense_scales=(0.75, 1.25)), True),
    ("predict_tile_dense + scales + tta", dict(dense_tile=96, dense_scales=(0.75, 1.25), dense_tta="d4"), True),
    ("predict_tile_dense + se", dict(dense_tile=96, dense_se="global"), False),
])
def test_sums_are_prob_is_the_table_of_design_8a4(kind, kw, is_prob):
    assert InferencePath(crop_size=25, **kw).sums_are_prob is is_prob


ARGV = ["x.py", "in/", "out/", "7"]


def test_take_flag_finds_the_flag_anywhere():
    number = lambda a, v: int(v)       # noqa: E731
    for i in range(len(ARGV) + 1):
        argv = ARGV[:i] + ["--n=3"] + ARGV[i:]
        assert cli._take_flag(argv, "--n", number) == (ARGV, 3)
        assert cli._take_flag(ARGV[:i] + ["--n"] + ARGV[i:], "--n", number, bare=0) == (ARGV, 0)
    assert cli._take_flag(ARGV + ["--n=3"], "--n", lambda a, v: (a, v)) == (ARGV, ("--n=3", "3"))
    assert cli._take_flag(ARGV + ["--nn=3", "--n=4"], "--n", number) == (ARGV + ["--nn=3"], 4)        # a longer flag is another flag


def test_take_flag_twice_raises():
    for twice in (["--n=3", "--n=4"], ["--n=3", "a", "--n=3"], ["--n", "--n=3"], ["--n", "--n"]):
        with pytest.raises(ValueError, match="--n given more than once"):
            cli._take_flag(ARGV + twice, "--n", lambda a, v: int(v), bare=0)
    with pytest.raises(ValueError, match="--n given more than once"):       # before the second value is looked at
        cli._take_flag(ARGV + ["--n=3", "--n=x"], "--n", lambda a, v: int(v))


def test_take_flag_bare_where_no_bare_form_exists_raises():
    def number(a, v):
        if not v.isdigit():
            raise ValueError("%s: expected --n=N" % a)
        return int(v)
    with pytest.raises(ValueError, match="--n: expected --n=N"):
        cli._take_flag(ARGV + ["--n"], "--n", number)
    with pytest.raises(ValueError, match="--n=: expected --n=N"):
        cli._take_flag(ARGV + ["--n="], "--n", number)
    for parse in (cli.parse_dense_tta, cli.parse_dense_scales, cli.parse_dense_se, cli.parse_score_maps, cli.parse_temperature,
                  cli.parse_class_weights, cli.parse_focal_gamma):
        flag = "--" + parse.__name__[len("parse_"):].replace("_", "-")
        with pytest.raises(ValueError, match=flag):
            parse(ARGV + [flag])


def test_take_flag_without_the_flag_returns_argv_unchanged_as_a_new_list():
    got, value = cli._take_flag(ARGV, "--n", lambda a, v: int(v), bare=0)
    assert value is None and got == ARGV and got is not ARGV and isinstance(got, list)
    got, value = cli._take_flag(tuple(ARGV), "--n", lambda a, v: int(v))
    assert value is None and got == ARGV and isinstance(got, list)
    for parse in (cli.parse_dense_tile, cli.parse_dense_tta, cli.parse_dense_scales, cli.parse_dense_se, cli.parse_score_maps,
                  cli.parse_calibrate_temperature, cli.parse_temperature, cli.parse_class_weights, cli.parse_focal_gamma):
        got, value = parse(ARGV)
        assert value is None and got == ARGV and got is not ARGV
