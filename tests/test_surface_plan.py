"""CPU: the host side of the surface-distance scores: the numpy statement of the exact distance transform and of the
table (tests/surface_ref.py) that the device tests are held to, on a map worked by hand and against scipy; metrics.surface_scores on
tables made by hand; patches.check_surface_tolerances / parse_surface_scores, the command-line flag, and the argument domains of the
entry points of csrc/distance.hip (host code: nothing is launched)."""
import ctypes

import numpy as np
import pytest

import surface_ref as R
from drs_amd import metrics as MT
from drs_amd import patches as P

INF, BINS = R.INF, R.BINS

HAND = np.array([[1, 1, 0, 0, 0],
                 [1, 1, 0, 0, 0],
                 [0, 0, 0, 0, 0],
                 [0, 0, 0, 0, 0],
                 [0, 0, 0, 0, 2]], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------- the reference itself
def test_ref_transform_on_a_hand_worked_map():
    block = np.array([[0, 0, 1, 4, 9], [0, 0, 1, 4, 9], [1, 1, 2, 5, 10], [4, 4, 5, 8, 13], [9, 9, 10, 13, 18]], dtype=np.int64)
    np.testing.assert_array_equal(R.distance2(HAND, R.CLASS, 1), block)
    # the contour of the block: (0, 0) has no neighbour of another byte inside the map -- the edge of the map is no boundary
    np.testing.assert_array_equal(R.sites(HAND, R.CONTOUR, 1), [[0, 1, 0, 0, 0], [1, 1, 0, 0, 0]] + [[0] * 5] * 3)
    contour = block.copy()
    contour[0, 0] = 1
    np.testing.assert_array_equal(R.distance2(HAND, R.CONTOUR, 1), contour)
    # everything that is not 0: the block and the lone 2 in the far corner
    np.testing.assert_array_equal(R.distance2(HAND, R.NOT_CLASS, 0),
                                  [[0, 0, 1, 4, 9], [0, 0, 1, 4, 9], [1, 1, 2, 5, 4], [4, 4, 5, 2, 1], [9, 9, 4, 1, 0]])
    assert (R.distance2(HAND, R.CLASS, 9) == INF).all()                   # no site: INF everywhere
    # through a veil: the one pixel the veil marks is the only site of its label, whatever the map holds there
    veil = np.zeros((5, 5), dtype=np.uint8)
    veil[2, 2] = 7
    yy, xx = np.mgrid[0:5, 0:5]
    np.testing.assert_array_equal(R.distance2(HAND, R.CLASS, 7, veil, 7), (yy - 2) ** 2 + (xx - 2) ** 2)
    np.testing.assert_array_equal(R.sites(HAND, R.CONTOUR, 0, veil, 7)[1:4, 1:4], [[0, 1, 0], [1, 0, 1], [0, 1, 0]])


def test_ref_bins_and_table_on_a_hand_worked_pair():
    assert [R.bin_of(D) for D in (0, 1, 2, 4, 5, 65025)] == [0, 4, 6, 8, 9, 1020]
    assert R.bin_of(1023 * 1023 + 1) == 4093 and R.bin_of(1100 * 1100) == 4400
    truth = np.zeros((5, 5), dtype=np.uint8)
    truth[:2, :2] = 1
    pred = np.zeros((5, 5), dtype=np.uint8)
    pred[:2, 2:4] = 1
    t = R.table(truth, pred, 2, -1)
    # class 1: truth contour (0, 1), (1, 0), (1, 1) at D = 1, 4, 1 of the prediction's; the prediction's four pixels at 1, 4, 1, 4
    assert t.shape == (2, 2, BINS + 2) and t[0, 1, 4] == 2 and t[0, 1, 8] == 1 and t[0, 1, BINS] == 2 * 1024 + 2048
    assert t[1, 1, 4] == 2 and t[1, 1, 8] == 2 and t[1, 1, BINS] == 2 * 1024 + 2 * 2048 and t[:, :, BINS + 1].sum() == 0
    assert t[0, 1, :BINS].sum() == 3 and t[1, 1, :BINS].sum() == 4
    # a class the prediction lacks: every pixel of its contour in the truth is unsited, nothing else of its rows moves
    none = R.table(truth, np.zeros_like(pred), 2, -1)
    assert none[0, 1, BINS + 1] == 3 and none[:, 1, :BINS + 1].sum() == 0 and none[1, 1, BINS + 1] == 0
    # the ignore label veils the prediction: where the truth says 1 = ignore, the prediction carries 1 too, and class 1 has no row
    ign = R.table(truth, pred, 2, 1)
    assert ign[:, 1].sum() == 0
    st, sp = R.contour_sets(truth, pred, 0, 1)
    np.testing.assert_array_equal(sp[:2], [[0, 0, 0, 0, 1], [0, 0, 0, 0, 1]])         # pred' = [1 1 1 1 0]: the 0 beside the block
    assert ign[0, 0, :BINS].sum() == st.sum() and ign[1, 0, :BINS].sum() == sp.sum()


def test_ref_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    truth, pred = R.synthetic_case(45, 131, 6, seed=3, ignore=6)
    for m, veil in ((truth, None), (pred, truth)):
        for mode in (R.CLASS, R.NOT_CLASS, R.CONTOUR):
            for cls in (0, 1, 6):
                s = R.sites(m, mode, cls, veil, None if veil is None else 6)
                want = np.full(s.shape, INF, dtype=np.int64)
                if s.any():
                    iy, ix = ndi.distance_transform_edt(~s, return_distances=False, return_indices=True)
                    yy, xx = np.mgrid[0:s.shape[0], 0:s.shape[1]]
                    want = (yy - iy) ** 2 + (xx - ix) ** 2                # integers from the nearest site's indices: no rounding
                np.testing.assert_array_equal(R.distance2_to(s), want, err_msg=str((mode, cls)))


# ------------------------------------------------------------------------------------------------------------- the scores
def _table(K):
    return np.zeros((2, K, BINS + 2), dtype=np.int64)


def test_surface_scores_on_hand_made_tables():
    t = _table(4)
    # class 0: 20 truth pixels, 19 at ceil(4 d) = 4 and one at 40: ceil(0.95 * 20) = 19 lands exactly on the edge of bin 4
    t[0, 0, 4], t[0, 0, 40], t[0, 0, BINS] = 19, 1, 30720
    t[1, 0, 8], t[1, 0, BINS] = 10, 20480
    # class 1: two maps' worth: one without the class in the prediction (5 unsited), one with it
    t[0, 1, 2], t[0, 1, BINS], t[0, 1, BINS + 1] = 5, 2560, 5
    t[1, 1, 2], t[1, 1, BINS] = 5, 2560
    # class 2: in the truth only; class 3: nowhere
    t[0, 2, BINS + 1] = 4
    s = MT.surface_scores(t, (1, 2))
    assert s["tolerances"] == (1, 2)
    np.testing.assert_array_equal(s["n_truth"], [20, 10, 4, 0])
    np.testing.assert_array_equal(s["n_pred"], [10, 5, 0, 0])
    np.testing.assert_array_equal(s["unsited_truth"], [0, 5, 4, 0])
    np.testing.assert_array_equal(s["unsited_pred"], [0, 0, 0, 0])
    np.testing.assert_array_equal(s["hd95"], [2.0, 0.5, np.nan, np.nan])
    np.testing.assert_array_equal(s["hd100"], [10.0, 0.5, np.nan, np.nan])
    np.testing.assert_array_equal(s["assd"], [51200 / 1024.0 / 30, 5120 / 1024.0 / 10, np.nan, np.nan])
    np.testing.assert_array_equal(s["saturated"], [False] * 4)
    assert s["nsd"].shape == (2, 4)
    np.testing.assert_array_equal(s["nsd"][0], [19 / 30, 10 / 15, 0.0, np.nan])       # the unsited pixels are in the denominator
    np.testing.assert_array_equal(s["nsd"][1], [29 / 30, 10 / 15, 0.0, np.nan])
    assert s["mean_hd95"] == 1.25 and s["mean_hd100"] == 5.25 and s["mean_assd"] == (50 / 30 + 0.5) / 2
    assert s["mean_nsd"] == [np.mean([19 / 30, 10 / 15, 0.0]), np.mean([29 / 30, 10 / 15, 0.0])]
    # one pixel more in the far bin moves the 95th percentile of direction 0 there: ceil(0.95 * 21) = 20 > 19
    t[0, 0, 40] = 2
    assert MT.surface_scores(t, (1,))["hd95"][0] == 10.0


def test_surface_scores_saturation_and_empty_tables():
    t = _table(2)
    t[0, 0, BINS - 1], t[0, 0, BINS] = 3, 3 * 1100 * 1024
    t[1, 0, 7], t[1, 0, BINS] = 3, 3 * 1792
    s = MT.surface_scores(t, (255,))
    assert s["saturated"].tolist() == [True, False] and s["hd95"][0] == (BINS - 1) / 4.0 and np.isnan(s["hd95"][1])
    assert s["nsd"][0, 0] == 0.5 and s["assd"][0] == (3 * 1100 + 3 * 1.75) / 6
    e = MT.surface_scores(_table(3), P.SURFACE_DEFAULT)
    assert np.isnan(e["mean_assd"]) and np.isnan(e["mean_hd95"]) and all(np.isnan(v) for v in e["mean_nsd"]) and len(e["mean_nsd"]) == 4
    assert e["n_truth"].tolist() == [0, 0, 0] and not e["saturated"].any()


@pytest.mark.parametrize("bad", [np.zeros((2, 3, BINS + 1), dtype=np.int64), np.zeros((1, 3, BINS + 2), dtype=np.int64),
                                 np.zeros((2, 3, BINS + 2)), np.full((2, 3, BINS + 2), -1, dtype=np.int64),
                                 np.zeros((2, BINS + 2), dtype=np.int64)])
def test_surface_scores_refuses_a_malformed_table(bad):
    with pytest.raises(ValueError, match="surface table"):
        MT.surface_scores(bad, (1,))


def test_scores_of_the_reference_table_are_the_definitions():
    """the scores of a small pair from the table against the same scores from the sorted distances themselves"""
    truth, pred = R.synthetic_case(40, 52, 3, seed=5)
    s = MT.surface_scores(R.table(truth, pred, 3, -1), (1, 3))
    for c in range(3):
        st, sp = R.contour_sets(truth, pred, c, -1)
        assert st.any() and sp.any()
        d0, d1 = np.sqrt(np.sort(R.distance2_to(sp)[st])), np.sqrt(np.sort(R.distance2_to(st)[sp]))
        assert s["n_truth"][c] == len(d0) and s["n_pred"][c] == len(d1)
        q = lambda d: np.ceil(4 * d[int(np.ceil(0.95 * len(d))) - 1]) / 4
        assert s["hd95"][c] == max(q(d0), q(d1)) and s["hd100"][c] == np.ceil(4 * max(d0[-1], d1[-1])) / 4
        assert abs(s["assd"][c] - (d0.sum() + d1.sum()) / (len(d0) + len(d1))) < 1.0 / 1024
        for i, tol in enumerate((1, 3)):
            assert s["nsd"][i][c] == ((d0 <= tol).sum() + (d1 <= tol).sum()) / (len(d0) + len(d1))


# ------------------------------------------------------------------------------------------------------------- the option's values
def test_check_surface_tolerances_and_parse():
    assert P.SURFACE_DEFAULT == (1, 2, 4, 8) == P.check_surface_tolerances(P.SURFACE_DEFAULT)
    assert P.check_surface_tolerances([3]) == (3,) and P.check_surface_tolerances(np.array([1, 255])) == (1, 255)
    got = P.check_surface_tolerances((np.int64(2), 5))
    assert got == (2, 5) and all(type(d) is int for d in got)
    assert P.check_surface_tolerances(list(range(1, 9))) == tuple(range(1, 9))
    assert P.parse_surface_scores("1,2,4,8") == (1, 2, 4, 8) and P.parse_surface_scores("255") == (255,)


@pytest.mark.parametrize("bad, names", [
    ((), "()"), ([], "[]"), ((2, 1), "1"), ((1, 1), "1"), ((0,), "0"), ((1, 256), "256"), (tuple(range(1, 10)), "9"), ((1, 2.0), "2.0"),
    ((1.5,), "1.5"), ((True,), "True"), ("1,2", "1,2"), (None, "None"), (4, "4"), ((1, "2"), "'2'"), ((-1, 2), "-1"),
])
def test_check_surface_tolerances_names_the_offender(bad, names):
    with pytest.raises(ValueError) as e:
        P.check_surface_tolerances(bad)
    assert names in str(e.value) and "1..255" in str(e.value), str(e.value)


@pytest.mark.parametrize("bad", ["", "2,1", "1,1", "0", "256", "1,2,3,4,5,6,7,8,9", "1.5", "1, 2", " 1", "1,", ",1", "a", "1,-2", "+1", None, 3])
def test_parse_surface_scores_refuses(bad):
    with pytest.raises(ValueError):
        P.parse_surface_scores(bad)


# ------------------------------------------------------------------------------------------------------------- the command line
ARGV = ["x.py", "a", "b"]
MAIN_ARGV = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
             "single_fixed", "25", "acc"]


def test_cli_parse_surface_scores_anywhere_in_argv():
    from drs_amd import cli
    got, value = cli.parse_surface_scores(ARGV)
    assert value is None and got == ARGV and got is not ARGV
    assert cli.parse_surface_scores(["--surface-scores"] + ARGV) == (ARGV, (1, 2, 4, 8))                   # the bare flag
    assert cli.parse_surface_scores(["x.py", "a", "--surface-scores=2,3,200", "b"]) == (ARGV, (2, 3, 200))
    assert cli.parse_boundary_scores(["--surface-scores"] + ARGV)[1] is None                               # another option
    for bad, say in ((["--surface-scores", "--surface-scores=2"], "more than once"), (["--surface-scores=1"] * 2, "more than once"),
                     (["--surface-scores="], "--surface-scores=t0,t1,..."), (["--surface-scores=2,1"], "ascending"),
                     (["--surface-scores=1,x"], "--surface-scores=t0,t1,..."), (["--surface-scores=256"], "1..255"),
                     (["--surface-scores=0.5"], "integers")):
        with pytest.raises(ValueError) as e:
            cli.parse_surface_scores(ARGV + bad)
        assert say in str(e.value), (bad, str(e.value))


def test_cli_flag_without_a_validating_run_exits():
    from drs_amd import cli
    from drs_amd.net import NoComm
    for tail, say in ((["training", "--surface-scores"], "--surface-scores applies to the validate_test process only"),
                      (["generate_final_maps", "--surface-scores=1,2"], "--surface-scores applies to the validate_test process only"),
                      (["validate_test", "--surface-scores=3,2"], "--surface-scores=t0,t1,..."),
                      (["validate_test", "--surface-scores", "--surface-scores"], "more than once")):
        with pytest.raises(SystemExit) as e:
            cli.main(MAIN_ARGV + tail, device="cpu", comm=NoComm())
        assert say in str(e.value), (tail, str(e.value))


class _Reached(Exception):
    pass


@pytest.mark.parametrize("flags, want", [([], "absent"), (["--surface-scores"], (1, 2, 4, 8)), (["--surface-scores=1,30", "--sieve=4"], (1, 30))])
def test_cli_flag_reaches_validate_test(monkeypatch, tmp_path, flags, want):
    """main parses, loads the synthetic tiles and calls loops.validate_test(..., surface_scores=...): the net and the checkpoint are
    stand-ins, the loop itself is intercepted.  Without the flag the loop is called without the argument at all."""
    from drs_amd import cli, loops, net as net_mod
    from drs_amd.net import NoComm
    import inspect
    assert inspect.signature(loops.validate_test).parameters["surface_scores"].default is None       # (the loop itself, not the stand-in)
    seen = {}

    def loop(*args, **kw):
        seen.update(kw)
        raise _Reached()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(net_mod, "DilatedNet", lambda *a, **k: object())
    monkeypatch.setattr(loops, "load_checkpoint", lambda *a, **k: None)
    monkeypatch.setattr(loops, "rank0_call", lambda comm, fn, what: (np.zeros(3), np.ones(3)))
    monkeypatch.setattr(loops, "validate_test", loop)
    argv = list(MAIN_ARGV)
    argv[1], argv[2], argv[3] = "synthetic:30x32x5/vaihingen/", str(tmp_path) + "/", "model-7"
    with pytest.raises(_Reached):
        cli.main(argv + ["validate_test"] + flags, device="cpu", comm=NoComm())
    assert seen.get("surface_scores", "absent") == want
    assert ("sieve" in seen) == ("--sieve=4" in flags) and "boundary_scores" not in seen and "object_scores" not in seen


def test_validate_test_refuses_bad_tolerances_before_it_touches_the_net():
    from drs_amd import loops
    with pytest.raises(ValueError, match="256"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, surface_scores=(1, 256))
    with pytest.raises(ValueError, match="surface tolerances"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, surface_scores=True)


def test_surface_str():
    from drs_amd import loops
    t = _table(2)
    t[0, 0, 4], t[0, 0, BINS], t[1, 0, 8], t[1, 0, BINS], t[0, 1, BINS + 1] = 2, 2048, 1, 2048, 3
    line = loops._surface_str(MT.surface_scores(t, (1, 2)))
    assert line == ("Surface tau= 1 2 Truth Contour= [2 3] Predicted Contour= [1 0] Unsited= [0 3] [0 0] ASSD= [1.333333 nan] "
                    "HD95= [2.000000 nan] Saturated= [0 0] HD100= [2.000000 nan] NSD= [0.666667 0.000000] [1.000000 0.000000] "
                    "Mean ASSD= 1.333333 Mean HD95= 2.000000 Mean NSD= 0.333333 0.500000")


# ------------------------------------------------------------------------------------------------------------- the entry points' checks
ERR_ARG = 1
p0, p1, p2, p3 = [0x10000 + 0x1000 * i for i in range(4)]                # dummy device pointers: host code never dereferences them
BIG = 1 << 40
DT_GOOD = [("map", p0), ("veil", p1), ("veil_label", 6), ("h", 40), ("w", 52), ("mode", 2), ("cls", 3), ("d2", p2), ("scratch", p3),
           ("scratch_bytes", BIG)]
SHAPE_BAD = [dict(h=0), dict(w=0), dict(h=-40), dict(w=-52), dict(h=32769), dict(w=32769), dict(h=32768, w=16384), dict(h=1 << 20, w=1 << 20)]
DT_BAD = SHAPE_BAD + [dict(map=None), dict(d2=None), dict(scratch=None), dict(mode=-1), dict(mode=3), dict(cls=-1), dict(cls=256),
                      dict(veil_label=-1), dict(veil_label=256), dict(scratch_bytes=0)]
SF_GOOD = [("truth", p0), ("pred", p1), ("h", 40), ("w", 52), ("K", 6), ("ignore_label", 6), ("table", p2), ("scratch", p3),
           ("scratch_bytes", BIG)]
SF_BAD = SHAPE_BAD + [dict(truth=None), dict(pred=None), dict(table=None), dict(scratch=None), dict(K=1), dict(K=9), dict(K=-6),
                      dict(ignore_label=-2), dict(ignore_label=256), dict(scratch_bytes=0)]


def _call(lib, name, args, change):
    a = dict(args)
    a.update(change)
    return getattr(lib, name)(*[a[k] for k, _ in args], None)


@pytest.mark.parametrize("name, good, bad, query", [("drs_distance_transform", DT_GOOD, DT_BAD, "drs_distance_scratch_bytes"),
                                                    ("drs_surface_histogram", SF_GOOD, SF_BAD, "drs_surface_scratch_bytes")])
def test_entry_points_reject_every_violation_of_their_domain(name, good, bad, query):
    """Argument validation is host code: every single-argument violation returns exactly DRS_ERR_ARG without touching the device (a
    call that passed validation would launch on the dummy pointers).  The scratch one byte short is a violation too."""
    from drs_amd import _lib
    lib = _lib.load()
    short = dict(scratch_bytes=_lib.query(query, 40, 52) - 1)
    wrong = [(change, rc) for change in bad + [short] for rc in [_call(lib, name, good, change)] if rc != ERR_ARG]
    assert not wrong, "%s: not DRS_ERR_ARG for %r" % (name, wrong)
    if name == "drs_distance_transform":                                  # without a veil its label is not looked at
        assert _call(lib, name, good, dict(veil=None, veil_label=-1, h=0)) == ERR_ARG


def test_scratch_queries_are_pure():
    from drs_amd import _lib
    for name in ("drs_distance_scratch_bytes", "drs_surface_scratch_bytes"):
        assert name in _lib.SIGNATURES
        for h, w in ((0, 5), (5, 0), (-1, 5), (32769, 1), (1, 32769), (32768, 16384)):
            assert _lib.query(name, h, w) == 0, (name, h, w)
        small, large = _lib.query(name, 40, 52), _lib.query(name, 32768, 8192)
        assert 0 < small < large and _lib.query(name, 1, 1) > 0 and _lib.query(name, 1, 32768) > 0 and _lib.query(name, 32768, 1) > 0
    assert _lib.query("drs_distance_scratch_bytes", 6000, 6000) <= 11 * 6000 * 6000
    assert _lib.query("drs_surface_scratch_bytes", 6000, 6000) <= 32 * 6000 * 6000
    for name in ("drs_distance_transform", "drs_surface_histogram"):
        assert name in _lib.SIGNATURES
