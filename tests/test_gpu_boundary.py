"""-m gpu: the boundary-quality counts (include/drs.h drs_boundary_distance / drs_boundary_histogram;
loops.boundary_histogram, validate_test's boundary_scores) against their numpy statement tests/boundary_ref.py.

Every comparison is exact integer equality: the rule is integer arithmetic, there are no tolerances and no excluded pixels."""
import ctypes

import numpy as np
import pytest
import torch

import boundary_ref

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

# (h, w, K, distances, ignore): ragged against any tile up to 64 in both axes; a map smaller than the window; one-pixel-wide maps;
# the largest table at full reach with ignore < K; no boundary anywhere
SHAPES = [(45, 131, 6, (1, 2, 4, 8), 6), (5, 7, 2, (8,), -1), (1, 40, 3, (1, 3), -1), (40, 1, 3, (1, 3), -1),
          (33, 65, 8, (1, 2, 3, 4, 6, 8, 12, 16), 7), (64, 64, 6, (1, 2, 4, 8), 6)]
IDS = ["45x131-K6", "5x7-K2", "1x40-K3", "40x1-K3", "33x65-K8-R16", "64x64-uniform"]
UNIFORM = SHAPES[-1]
_CASES = {}


def _case(shape):
    """the two maps and the reference table of a shape, computed once and shared by the tests (read-only)"""
    if shape not in _CASES:
        h, w, K, distances, ignore = shape
        if shape == UNIFORM:
            truth, pred = np.full((h, w), 2, dtype=np.uint8), np.full((h, w), 2, dtype=np.uint8)
        else:
            truth, pred = boundary_ref.synthetic_case(h, w, K, seed=0, ignore=ignore)
        hist = boundary_ref.histogram(truth, pred, K, ignore, distances)
        for a in (truth, pred, hist):
            a.setflags(write=False)
        _CASES[shape] = dict(truth=truth, pred=pred, hist=hist)
    return _CASES[shape]


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _distance(m, R):
    from drs_amd import _lib
    h, w = m.shape
    out = torch.full((h * w,), 12345, dtype=torch.int16, device=DEV)                 # (uint16 bits in an int16 tensor)
    md = dev(np.array(m).reshape(-1))                                                # (a copy: the shared inputs are read-only)
    _lib.call("drs_boundary_distance", md.data_ptr(), h, w, R, out.data_ptr(), stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16).reshape(h, w)


def _histogram(truth, pred, K, ignore, distances, hist=None):
    from drs_amd import _lib
    h, w = truth.shape
    n = len(distances)
    hist = torch.zeros((n + 1) * (n + 1) * K * K, dtype=torch.int64, device=DEV) if hist is None else hist
    d = _ints(distances)
    t, p = dev(np.array(truth).reshape(-1)), dev(np.array(pred).reshape(-1))
    _lib.call("drs_boundary_histogram", t.data_ptr(), p.data_ptr(), h, w, K, ignore, ctypes.addressof(d), n, hist.data_ptr(), stream())
    torch.cuda.synchronize()
    return hist.cpu().numpy().reshape(n + 1, n + 1, K, K)


# ------------------------------------------------------------------------------------------------------------- 1. the distance field
@pytest.mark.parametrize("which", ["truth", "pred"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_distance_field(shape, which):
    m = _case(shape)[which]
    for R in sorted({shape[3][-1], 16}):
        np.testing.assert_array_equal(_distance(m, R), boundary_ref.distance2_u16(m, R), err_msg="R=%d" % R)
    if shape == UNIFORM:
        assert (_distance(m, 16) == 65535).all()


def test_distance_ties_fall_into_the_inclusive_bin():
    distances = (1, 2, 3, 5)
    for off, d2, want_bin in (((1, 1), 2, 1), ((1, 3), 10, 3), ((3, 4), 25, 3), ((3, 1), 10, 3), ((4, 3), 25, 3), ((0, 3), 9, 2)):
        truth = np.zeros((20, 24), dtype=np.uint8)
        truth[9 + off[0], 11 + off[1]] = 1                                           # a lone other byte at that offset of (9, 11)
        pred = np.zeros_like(truth)
        assert _distance(truth, 5)[9, 11] == d2 == boundary_ref.distance2(truth, 5)[9, 11]
        # count (9, 11) alone: every other pixel of the prediction is an out-of-range byte
        pred[:] = 9
        pred[9, 11] = 0
        hist = _histogram(truth, pred, 2, -1, distances)
        np.testing.assert_array_equal(hist, boundary_ref.histogram(truth, pred, 2, -1, distances))
        assert hist.sum() == 1 and hist[want_bin, 0, 0, 0] == 1, (off, np.argwhere(hist))


# ------------------------------------------------------------------------------------------------------------- 2. the table
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_histogram(shape):
    h, w, K, distances, ignore = shape
    c = _case(shape)
    got = _histogram(c["truth"], c["pred"], K, ignore, distances)
    np.testing.assert_array_equal(got, c["hist"])
    n = len(distances)
    if shape == UNIFORM:
        assert got[n, n, 2, 2] == h * w == got.sum()
    if shape == SHAPES[0]:
        assert (got.sum(axis=(2, 3)) > 0).all()                                      # every block of bins is exercised


def test_counters_are_added_to():
    h, w, K, distances, ignore = SHAPES[0]
    c = _case(SHAPES[0])
    n = len(distances)
    rng = np.random.default_rng(1)
    before = rng.integers(1, 1 << 40, size=(n + 1, n + 1, K, K), dtype=np.int64)
    hist = dev(before.reshape(-1))
    _histogram(c["truth"], c["pred"], K, ignore, distances, hist)
    got = _histogram(c["truth"], c["pred"], K, ignore, distances, hist)
    np.testing.assert_array_equal(got, before + 2 * c["hist"])


def test_prediction_bytes_out_of_range_are_not_counted_but_still_differ():
    h, w, K, distances, ignore = SHAPES[0]
    c = _case(SHAPES[0])
    pred = np.array(c["pred"])
    pred[10:14, 20:90] = 200                                                         # a bar of a byte >= K through several objects
    pred[30, 5] = K
    want = boundary_ref.histogram(c["truth"], pred, K, ignore, distances)
    got = _histogram(c["truth"], pred, K, ignore, distances)
    np.testing.assert_array_equal(got, want)
    counted = boundary_ref.counted(c["truth"], pred, K, ignore)
    assert got.sum() == counted.sum() < boundary_ref.counted(c["truth"], c["pred"], K, ignore).sum()
    # the pixels beside the bar are at distance 1 of a different byte in the prediction: more of them than without it
    assert got[:, 0].sum() > c["hist"][:, 0].sum()
    np.testing.assert_array_equal(_distance(pred, 8), boundary_ref.distance2_u16(pred, 8))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_table_sums_to_drs_confusion(shape):
    from drs_amd import _lib
    h, w, K, distances, ignore = shape
    c = _case(shape)
    t, p = dev(np.array(c["truth"]).reshape(-1)), dev(np.array(c["pred"]).reshape(-1))
    conf = torch.zeros(K * K, dtype=torch.int32, device=DEV)
    n = len(distances)
    hist = torch.zeros((n + 1, n + 1, K, K), dtype=torch.int64, device=DEV)
    d = _ints(distances)
    _lib.call("drs_confusion", t.data_ptr(), p.data_ptr(), None, h * w, K, ignore, conf.data_ptr(), stream())
    _lib.call("drs_boundary_histogram", t.data_ptr(), p.data_ptr(), h, w, K, ignore, ctypes.addressof(d), n, hist.data_ptr(), stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hist.cpu().numpy().sum(axis=(0, 1)), conf.cpu().numpy().reshape(K, K))


def test_loops_boundary_histogram_is_a_thin_call():
    from drs_amd import loops
    h, w, K, distances, ignore = SHAPES[0]
    c = _case(SHAPES[0])
    t, p = dev(np.array(c["truth"]).reshape(-1)), dev(np.array(c["pred"]).reshape(-1))
    hist = loops.boundary_histogram(t, p, h, w, K, ignore, distances)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (5, 5, K, K) and hist.device == t.device
    again = loops.boundary_histogram(t, p, h, w, K, ignore, list(distances), hist=hist, stream=stream())
    torch.cuda.synchronize()
    assert again is hist
    np.testing.assert_array_equal(hist.cpu().numpy(), 2 * c["hist"])
    with pytest.raises(ValueError, match="int64"):
        loops.boundary_histogram(t, p, h, w, K, ignore, distances, hist=torch.zeros(5 * 5 * K * K, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="17"):
        loops.boundary_histogram(t, p, h, w, K, ignore, (1, 17))


# ------------------------------------------------------------------------------------------------------------- 3. arguments
def test_rejected_arguments_return_err_arg_and_leave_the_table_alone():
    from drs_amd import _lib
    h, w, K, distances, ignore = SHAPES[1]
    c = _case(SHAPES[1])
    t, p = dev(np.array(c["truth"]).reshape(-1)), dev(np.array(c["pred"]).reshape(-1))
    n = len(distances)
    hist = torch.full(((n + 1) * (n + 1) * K * K,), 7, dtype=torch.int64, device=DEV)
    d2 = torch.full((h * w,), 77, dtype=torch.int16, device=DEV)
    ok = _ints(distances)
    good = dict(truth=t.data_ptr(), pred=p.data_ptr(), h=h, w=w, K=K, ignore=ignore, distances=ctypes.addressof(ok), n=n, hist=hist.data_ptr())
    lists = [_ints(v) for v in ((2, 1), (3, 3), (0, 2), (1, 17), (-4, 2))]
    bad = [dict(truth=None), dict(pred=None), dict(distances=None), dict(hist=None), dict(h=0), dict(w=0), dict(w=-1), dict(K=1), dict(K=9),
           dict(n=0), dict(n=9), dict(h=1 << 20, w=1 << 20)] + [dict(distances=ctypes.addressof(v), n=2) for v in lists]
    for kw in bad:
        a = dict(good, **kw)
        assert _lib.query("drs_boundary_histogram", *[a[k] for k in good], stream()) == 1, kw
    for args in ((None, h, w, 2, d2.data_ptr()), (t.data_ptr(), h, w, 2, None), (t.data_ptr(), 0, w, 2, d2.data_ptr()),
                 (t.data_ptr(), h, 0, 2, d2.data_ptr()), (t.data_ptr(), h, w, 0, d2.data_ptr()), (t.data_ptr(), h, w, 17, d2.data_ptr()),
                 (t.data_ptr(), 1 << 20, 1 << 20, 2, d2.data_ptr())):
        assert _lib.query("drs_boundary_distance", *args, stream()) == 1, args
    torch.cuda.synchronize()
    assert (hist == 7).all() and (d2 == 77).all()                                    # nothing was launched
    assert _lib.query("drs_boundary_histogram", *[good[k] for k in good], stream()) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(hist.cpu().numpy().reshape(n + 1, n + 1, K, K), 7 + c["hist"])


# ------------------------------------------------------------------------------------------------------------- 4. the loop
CH, K6 = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
DIST = (1, 2, 4)
CRF = dict(iters=2, radius=3, step=1, w_app=4.0, theta_xy=8.0, theta_rgb=0.08, w_smooth=2.0, theta_s=2.0)


def _net(seed=5):
    """test_gpu_crf's net: random moving statistics and a classifier scaled so that the logits have a spread"""
    from drs_amd.net import DilatedNet
    rng = np.random.default_rng(seed)
    d = DilatedNet("dilated_grsl", CH, K6, 0.005, b_max=6, s_max=25, device=DEV, seed=seed)
    for n in d.variable_names():
        v = d.get_variable(n)
        if n.endswith("moving_mean"):
            d.set_variable(n, (rng.normal(size=v.shape) * 0.1).astype(np.float32))
        elif n.endswith("moving_variance"):
            d.set_variable(n, rng.uniform(0.5, 2.0, size=v.shape).astype(np.float32))
    d.set_variable("conv_classifier/weights", d.get_variable("conv_classifier/weights") * np.float32(16.0))
    return d


def _ref_tables(labs, maps):
    return [boundary_ref.histogram(lab, m, K6, 6, DIST) for lab, m in zip(labs, maps)]


def test_validate_test_reports_the_tables_of_the_maps_it_scored(capsys):
    from drs_amd import loops, metrics as MT
    from drs_amd.synthetic import make_tile
    tiles, labs = zip(*[make_tile(h, w, CH, K6, seed=s, n_seeds=30) for h, w, s in ((44, 50, 21), (37, 61, 22))])
    tiles, labs = list(tiles), list(labs)
    d = _net()
    capsys.readouterr()
    cm0, maps0 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7)
    text0 = capsys.readouterr().out
    cm1, maps1, extra = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, boundary_scores=DIST)
    text1 = capsys.readouterr().out
    assert set(extra) == {"boundary"}                                                # no score-map keys without score_maps
    b = extra["boundary"]
    per_map = _ref_tables(labs, maps1)
    assert b["hist"].dtype == np.int64 and b["hist"].shape == (4, 4, K6, K6)
    np.testing.assert_array_equal(b["hist"], per_map[0] + per_map[1])
    np.testing.assert_array_equal(b["confusion"], cm1)
    np.testing.assert_array_equal(cm0, cm1)
    for m0, m1 in zip(maps0, maps1):
        np.testing.assert_array_equal(m0, m1)
    assert len(b["per_map"]) == 2 and b["distances"] == DIST
    for got, table in zip(b["per_map"], per_map):
        want = MT.boundary_scores(table, DIST)
        np.testing.assert_array_equal(got["confusion"], want["confusion"])
        assert [x["count"] for x in got["bands"]] == [x["count"] for x in want["bands"]]
        assert [x["boundary_iou"] for x in got["bands"]] == [x["boundary_iou"] for x in want["bands"]]
    assert b["bands"][-1]["count"] > 0 and 0.0 < b["mean_iou"] <= 1.0
    # the Boundary lines: one per map and one for all maps, each after its reference-format line; everything else byte for byte
    lines0, lines1 = text0.splitlines(), text1.splitlines()
    mine = [i for i, line in enumerate(lines1) if ": Boundary d= 1 2 4 Band Pixels= " in line]
    assert len(mine) == 3 and lines0
    assert [line for i, line in enumerate(lines1) if i not in mine] == lines0
    for i, who in zip(mine, ("Test Map a: ", "Test Map b: ", "Test ALL MAPS: ")):
        assert lines1[i].startswith("---- Iter 7 -- " + who + "Boundary d= ")
        assert lines1[i - 1].startswith("---- Iter 7 -- " + who + "Overall Accuracy= ")
    last = lines1[mine[-1]]
    assert last.startswith("---- Iter 7 -- Test ALL MAPS: Boundary d= 1 2 4 Band Pixels= " + " ".join(str(x["count"]) for x in b["bands"]))
    assert last.endswith(" Mean IoU= " + "{:.6f}".format(b["mean_iou"]))
    for key in (" Band Accuracy= ", " Boundary IoU= ", " Boundary IoU per class (d= 4)= ", " IoU per class= "):
        assert key in last
    # with score maps the keys of both reports are there, and the Boundary line follows the Calibration line
    _, _, both = loops.validate_test(d, tiles[:1], labs[:1], ["a"], 6, MEAN, STD, 25, 7, boundary_scores=DIST, score_maps=("margin",))
    lines = [s for s in capsys.readouterr().out.splitlines() if s.startswith("---- Iter 7 -- Test ")]
    assert {"boundary", "scores", "reliability", "calibration"} <= set(both)
    assert [("Calibration ECE=" in s, ": Boundary d=" in s) for s in lines] == [(False, False), (True, False), (False, True)] * 2
    np.testing.assert_array_equal(both["boundary"]["hist"], per_map[0])


def test_validate_test_with_a_crf_counts_the_refined_maps(capsys):
    from drs_amd import loops
    from drs_amd.synthetic import make_tile
    tile, lab = make_tile(44, 50, CH, K6, seed=21, n_seeds=30)
    d = _net()
    _, plain = loops.validate_test(d, [tile], [lab], ["a"], 6, MEAN, STD, 25, 7)
    cm, maps, extra = loops.validate_test(d, [tile], [lab], ["a"], 6, MEAN, STD, 25, 7, boundary_scores=DIST, crf=CRF)
    capsys.readouterr()
    assert (maps[0] != plain[0]).any()                                               # the CRF moved labels, so the two tables differ
    np.testing.assert_array_equal(extra["boundary"]["hist"], _ref_tables([lab], maps)[0])
    assert (extra["boundary"]["hist"] != _ref_tables([lab], plain)[0]).any()
    np.testing.assert_array_equal(extra["boundary"]["confusion"], cm)
