"""CPU: the host side of the boundary-quality scores: the numpy statement of the distance field, the bins and the
table (tests/boundary_ref.py) that the device tests are held to, metrics.boundary_scores / iou_per_class / mean_iou on tables worked by
hand, patches.check_boundary_distances / parse_boundary_scores, the command-line flag, and the argument checks of the two entry points
(host code: no launch)."""
import ctypes

import numpy as np
import pytest

import boundary_ref
from drs_amd import metrics as MT
from drs_amd import patches as P

INF = boundary_ref.INF


# ------------------------------------------------------------------------------------------------------------- the reference itself
def test_ref_distance_on_a_hand_worked_map():
    m = np.array([[0, 0, 0, 0, 2],
                  [0, 0, 0, 0, 0],
                  [0, 1, 0, 0, 0],
                  [0, 0, 0, 0, 0],
                  [0, 0, 0, 0, 0]], dtype=np.uint8)
    # the 1 at (2, 1) is in the window of columns 0..3, the 2 at (0, 4) in that of rows 0..2 and columns 2..4; (3, 4) and (4, 4) see
    # neither; the bottom and right edges of the map are not boundaries
    want2 = np.array([[5, 4, 4, 1, 1],
                      [2, 1, 2, 2, 1],
                      [1, 1, 1, 4, 4],
                      [2, 1, 2, 5, INF],
                      [5, 4, 5, 8, INF]], dtype=np.int64)
    np.testing.assert_array_equal(boundary_ref.distance2(m, 2), want2)
    want1 = np.array([[INF, INF, INF, 1, 1],
                      [2, 1, 2, 2, 1],
                      [1, 1, 1, INF, INF],
                      [2, 1, 2, INF, INF],
                      [INF, INF, INF, INF, INF]], dtype=np.int64)
    np.testing.assert_array_equal(boundary_ref.distance2(m, 1), want1)
    np.testing.assert_array_equal(boundary_ref.distance2_u16(m, 1)[4], 65535)
    # bins: D2 <= d^2 is inclusive; what no distance reaches lands in bin n
    np.testing.assert_array_equal(boundary_ref.bins(want2, (1, 2)), [[2, 1, 1, 0, 0], [1, 0, 1, 1, 0], [0, 0, 0, 1, 1], [1, 0, 1, 2, 2],
                                                                       [2, 1, 2, 2, 2]])


def test_ref_distance_against_scipy_edt():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:40, 0:56]
    m = (((yy - 17) ** 2 + (xx - 22) ** 2 < 120) | ((yy - 30) ** 2 * 3 + (xx - 44) ** 2 < 90)).astype(np.uint8)
    m[rng.integers(0, 40, 5), rng.integers(0, 56, 5)] ^= 1
    R = 6
    got = boundary_ref.distance2(m, R)
    # per label: the distance to the nearest pixel of the complement.  scipy's transform knows no map edge either, so the two agree
    # on the whole map, its interior included; beyond R the window is a square and the disc says only "further than R"
    edt2 = np.where(m == 1, np.rint(ndi.distance_transform_edt(m == 1) ** 2), np.rint(ndi.distance_transform_edt(m == 0) ** 2)).astype(np.int64)
    near = edt2 <= R * R
    assert near[8:-8, 8:-8].any() and (~near)[8:-8, 8:-8].any()
    np.testing.assert_array_equal(got[near], edt2[near])
    assert (got[~near] > R * R).all()


def test_ref_table_is_populated_in_every_block_at_the_device_tests_shape():
    truth, pred = boundary_ref.synthetic_case(45, 131, 6, seed=0, ignore=6)
    hist = boundary_ref.histogram(truth, pred, 6, 6, (1, 2, 4, 8))
    blocks = hist.sum(axis=(2, 3))
    assert blocks.shape == (5, 5) and (blocks > 0).all(), blocks           # the device comparison cannot pass vacuously
    assert (truth == 6).any() and (np.diagonal(hist.sum(axis=(0, 1))) > 0).sum() >= 3
    np.testing.assert_array_equal(hist.sum(axis=(0, 1)), boundary_ref.confusion(truth, pred, 6, 6))
    assert hist.sum() == (truth != 6).sum()


def test_ref_bytes_are_just_bytes_and_the_edge_is_no_boundary():
    m = np.zeros((6, 9), dtype=np.uint8)
    assert (boundary_ref.distance2(m, 4) == INF).all()                     # uniform: nothing differs, the edge least of all
    m[:, 4] = 200                                                          # any byte is a label
    d = boundary_ref.distance2(m, 4)
    np.testing.assert_array_equal(d[0], [16, 9, 4, 1, 1, 1, 4, 9, 16])
    truth, pred = m.copy(), np.zeros_like(m)
    truth[truth == 200] = 7
    hist = boundary_ref.histogram(truth, pred, 3, 7, (1, 4))               # the ignore band is not counted, its neighbours are near it
    assert hist.sum() == 6 * 8 and hist[0, 2, 0, 0] == 12 and hist[1, 2, 0, 0] == 36 and hist[2].sum() == 0


# ------------------------------------------------------------------------------------------------------------- metrics
H00 = [[3, 1, 0], [0, 2, 0], [0, 0, 0]]
H01 = [[1, 0, 0], [1, 0, 0], [0, 0, 0]]
H10 = [[0, 2, 0], [0, 1, 0], [0, 0, 0]]
H11 = [[10, 0, 0], [1, 20, 0], [0, 0, 0]]


def _check_band_d2(band):
    # T = H00 + H01 = [[4, 1, 0], [1, 2, 0], [0, 0, 0]]
    np.testing.assert_array_equal(band["confusion"], [[4, 1, 0], [1, 2, 0], [0, 0, 0]])
    assert band["d"] == 2 and band["count"] == 8
    assert band["accuracy"] == pytest.approx(6 / 8, abs=1e-15)
    assert band["normalized_accuracy"] == pytest.approx((4 / 5 + 2 / 3 + 0) / 3, abs=1e-15)
    # class 0: I = 3, G = 4 + 1 = 5, P = H00[:, 0] + H10[:, 0] = 3 + 0 -> 3 / 5;  class 1: I = 2, G = 3, P = (1 + 2) + (2 + 1) = 6 -> 2 / 7
    np.testing.assert_allclose(band["boundary_iou_per_class"], [3 / 5, 2 / 7, 0.0], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(band["boundary_iou_present"], [True, True, False])
    assert band["boundary_iou"] == pytest.approx((3 / 5 + 2 / 7) / 2, abs=1e-15)


def test_boundary_scores_on_a_hand_made_table():
    hist = np.array([[H00, H01], [H10, H11]], dtype=np.int64)
    s = MT.boundary_scores(hist, (2,))
    assert s["distances"] == (2,) and len(s["bands"]) == 1
    np.testing.assert_array_equal(s["confusion"], [[14, 3, 0], [2, 23, 0], [0, 0, 0]])
    np.testing.assert_array_equal(s["confusion"], hist.sum(axis=(0, 1)))
    np.testing.assert_allclose(s["iou_per_class"], [14 / 19, 23 / 28, 0.0], rtol=0, atol=1e-15)        # class 2 is absent
    assert s["mean_iou"] == pytest.approx((14 / 19 + 23 / 28) / 2, abs=1e-15)
    _check_band_d2(s["bands"][0])
    # an empty band in front: nothing lies within 1 pixel of a boundary in either map
    wide = np.zeros((3, 3, 3, 3), dtype=np.uint32)
    wide[1:, 1:] = hist
    s = MT.boundary_scores(wide, [1, 2])
    b = s["bands"][0]
    assert (b["d"], b["count"], b["accuracy"], b["normalized_accuracy"], b["boundary_iou"]) == (1, 0, 0.0, 0.0, 0.0)
    assert not b["boundary_iou_present"].any() and not b["boundary_iou_per_class"].any() and not b["confusion"].any()
    _check_band_d2(s["bands"][1])
    np.testing.assert_array_equal(s["confusion"], [[14, 3, 0], [2, 23, 0], [0, 0, 0]])
    # the last band of a table whose far bin is empty is the whole confusion matrix
    full = np.zeros((2, 2, 3, 3), dtype=np.int64)
    full[0, 0] = s["confusion"]
    s = MT.boundary_scores(full, (16,))
    np.testing.assert_allclose(s["bands"][0]["boundary_iou_per_class"], s["iou_per_class"], rtol=0, atol=0)
    assert s["bands"][0]["count"] == 42 and MT.boundary_scores(np.zeros((2, 2, 3, 3), dtype=np.int64), (3,))["mean_iou"] == 0.0


@pytest.mark.parametrize("bad, distances", [
    (np.zeros((2, 2, 3, 3)), (2,)), (np.zeros((3, 3, 3, 3), dtype=np.int64), (2,)), (np.zeros((2, 2, 3, 4), dtype=np.int64), (2,)),
    (np.zeros((2, 3, 3, 3), dtype=np.int64), (2,)), (np.zeros((2, 2, 9), dtype=np.int64), (2,)),
    (-np.ones((2, 2, 3, 3), dtype=np.int64), (2,)), (np.zeros((2, 2, 3, 3), dtype=np.int64), (1, 2)),
])
def test_boundary_scores_refuses_a_malformed_table(bad, distances):
    with pytest.raises(ValueError, match="boundary table"):
        MT.boundary_scores(bad, distances)


def test_iou_against_a_direct_computation():
    rng = np.random.default_rng(0)
    truth, pred = rng.integers(0, 5, 4000), rng.integers(0, 4, 4000)          # class 4 is never predicted, class 5 never occurs
    cm = np.zeros((6, 6), dtype=np.int64)
    np.add.at(cm, (truth, pred), 1)
    iou, present = MT.iou_per_class(cm)
    want = [np.sum((truth == c) & (pred == c)) / np.sum((truth == c) | (pred == c)) for c in range(5)]
    np.testing.assert_array_equal(present, [True] * 5 + [False])
    np.testing.assert_allclose(iou, want, rtol=0, atol=1e-15)
    assert iou[4] == 0.0 and MT.mean_iou(cm) == pytest.approx(np.mean(want), abs=1e-15)
    assert MT.mean_iou(np.zeros((3, 3), dtype=np.int64)) == 0.0 and len(MT.iou_per_class(np.zeros((3, 3)))[0]) == 0
    np.testing.assert_array_equal(MT.iou_per_class(cm)[1], MT.f1_per_class(cm)[1])          # one presence rule


# ------------------------------------------------------------------------------------------------------------- the option's values
def test_check_boundary_distances_and_parse():
    assert P.BOUNDARY_DEFAULT == (1, 2, 4, 8) == P.check_boundary_distances(P.BOUNDARY_DEFAULT)
    assert P.check_boundary_distances([3]) == (3,) and P.check_boundary_distances(np.array([1, 16])) == (1, 16)
    got = P.check_boundary_distances((np.int64(2), 5))
    assert got == (2, 5) and all(type(d) is int for d in got)
    assert P.check_boundary_distances(list(range(1, 9))) == tuple(range(1, 9))
    assert P.parse_boundary_scores("1,2,4,8") == (1, 2, 4, 8) and P.parse_boundary_scores("16") == (16,)
    assert P.parse_boundary_scores("1,2,3,4,6,8,12,16") == (1, 2, 3, 4, 6, 8, 12, 16)


@pytest.mark.parametrize("bad, names", [
    ((), "()"), ([], "[]"), ((2, 1), "1"), ((1, 1), "1"), ((0,), "0"), ((1, 17), "17"), (tuple(range(1, 10)), "9"), ((1, 2.0), "2.0"),
    ((1.5,), "1.5"), ((True,), "True"), ("1,2", "1,2"), (None, "None"), (4, "4"), ((1, "2"), "'2'"), ((-1, 2), "-1"),
])
def test_check_boundary_distances_names_the_offender(bad, names):
    with pytest.raises(ValueError) as e:
        P.check_boundary_distances(bad)
    assert names in str(e.value) and "1..16" in str(e.value), str(e.value)


@pytest.mark.parametrize("bad", ["", "2,1", "1,1", "0", "17", "1,2,3,4,5,6,7,8,9", "1.5", "1, 2", " 1", "1,", ",1", "a", "1,-2", "+1", None, 3])
def test_parse_boundary_scores_refuses(bad):
    with pytest.raises(ValueError):
        P.parse_boundary_scores(bad)


# ------------------------------------------------------------------------------------------------------------- the command line
ARGV = ["x.py", "a", "b"]
MAIN_ARGV = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
             "single_fixed", "25", "acc"]


def test_cli_parse_boundary_scores_anywhere_in_argv():
    from drs_amd import cli
    got, value = cli.parse_boundary_scores(ARGV)
    assert value is None and got == ARGV and got is not ARGV
    assert cli.parse_boundary_scores(["--boundary-scores"] + ARGV) == (ARGV, (1, 2, 4, 8))                 # the bare flag
    assert cli.parse_boundary_scores(["x.py", "a", "--boundary-scores=2,3,16", "b"]) == (ARGV, (2, 3, 16))
    for bad, say in ((["--boundary-scores", "--boundary-scores=2"], "more than once"), (["--boundary-scores=1"] * 2, "more than once"),
                     (["--boundary-scores="], "--boundary-scores=d0,d1,..."), (["--boundary-scores=2,1"], "ascending"),
                     (["--boundary-scores=1,x"], "--boundary-scores=d0,d1,..."), (["--boundary-scores=17"], "1..16"),
                     (["--boundary-scores=0.5"], "integers")):
        with pytest.raises(ValueError) as e:
            cli.parse_boundary_scores(ARGV + bad)
        assert say in str(e.value), (bad, str(e.value))


def test_cli_flag_without_a_validating_run_exits():
    from drs_amd import cli
    from drs_amd.net import NoComm
    for tail, say in ((["training", "--boundary-scores"], "--boundary-scores applies to the validate_test process only"),
                      (["generate_final_maps", "--boundary-scores=1,2"], "--boundary-scores applies to the validate_test process only"),
                      (["validate_test", "--boundary-scores=3,2"], "--boundary-scores=d0,d1,..."),
                      (["validate_test", "--boundary-scores", "--boundary-scores"], "more than once")):
        with pytest.raises(SystemExit) as e:
            cli.main(MAIN_ARGV + tail, device="cpu", comm=NoComm())
        assert say in str(e.value), (tail, str(e.value))


class _Reached(Exception):
    pass


@pytest.mark.parametrize("flags, want", [([], "absent"), (["--boundary-scores"], (1, 2, 4, 8)), (["--boundary-scores=1,3", "--crf"], (1, 3))])
def test_cli_flag_reaches_validate_test(monkeypatch, tmp_path, flags, want):
    """main parses, loads the synthetic tiles and calls loops.validate_test(..., boundary_scores=...): the net and the checkpoint are
    stand-ins, the loop itself is intercepted.  Without the flag the loop is called without the argument at all."""
    from drs_amd import cli, loops, net as net_mod
    from drs_amd.net import NoComm
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
    assert seen.get("boundary_scores", "absent") == want
    assert ("crf" in seen) == ("--crf" in flags)


def test_validate_test_refuses_bad_distances_before_it_touches_the_net():
    from drs_amd import loops
    with pytest.raises(ValueError, match="17"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, boundary_scores=(1, 17))
    with pytest.raises(ValueError, match="boundary distances"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, boundary_scores=True)


# ------------------------------------------------------------------------------------------------------------- the entry points' checks
def test_entry_points_reject_bad_arguments_before_any_launch():
    """Argument validation is host code: every rejected call returns DRS_ERR_ARG (raised as DrsError) without touching the device.
    Map and table pointers are dummies; a call that passed validation would launch."""
    from drs_amd import _lib
    _lib.load()
    p, q = 0x1000, 0x2000

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)
    ok = ints(1, 2, 4, 8)
    good = dict(truth=p, pred=p, h=40, w=50, K=6, ignore=6, distances=ctypes.addressof(ok), n=4, hist=q)
    lists = [ints(2, 1, 4, 8), ints(1, 2, 2, 8), ints(0, 2, 4, 8), ints(1, 2, 4, 17), ints(-1, 2, 4, 8)]
    bad = [dict(truth=None), dict(pred=None), dict(distances=None), dict(hist=None), dict(h=0), dict(w=0), dict(h=-3), dict(K=1), dict(K=9),
           dict(n=0), dict(n=9), dict(h=1 << 20, w=1 << 20)] + [dict(distances=ctypes.addressof(v)) for v in lists]
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(_lib.DrsError, match="DRS_ERR_ARG"):
            _lib.call("drs_boundary_histogram", *[a[k] for k in good], None)
    for args in ((None, 4, 4, 2, q), (p, 4, 4, 2, None), (p, 0, 4, 2, q), (p, 4, 0, 2, q), (p, 4, 4, 0, q), (p, 4, 4, 17, q),
                 (p, 1 << 20, 1 << 20, 2, q)):
        with pytest.raises(_lib.DrsError, match="DRS_ERR_ARG"):
            _lib.call("drs_boundary_distance", *args, None)
