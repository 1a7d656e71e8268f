"""-m gpu: the exact distance transform and the surface-distance table (include/drs.h drs_distance_transform /
drs_surface_histogram; loops.distance_transform, loops.surface_histogram, validate_test's surface_scores) against their numpy statement
tests/surface_ref.py.

Every comparison is exact integer equality: the rule is integer arithmetic, there are no tolerances and no excluded pixels.  Every raw
call runs with its outputs, its scratch and a guard region behind each filled with 0xA5, and checks the guards."""
import numpy as np
import pytest
import torch

import surface_ref as R

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

INF, BINS = R.INF, R.BINS
GUARD = 256
TILE, ROWS, WIDE = 64, 16, 256                   # csrc/distance.hip: the column strips' height; the rows and columns of the row pass's tile


def _guarded(nbytes, fill):
    """a uint8 device buffer of nbytes + GUARD bytes, all `fill`"""
    return torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device=DEV)


def _guard_ok(buf, nbytes, fill):
    return bool((buf[nbytes:] == fill).all().item())


def _transform(m, mode, cls, veil=None, veil_label=None, fill=0xA5):
    from drs_amd import _lib
    h, w = m.shape
    need = _lib.query("drs_distance_scratch_bytes", h, w)
    assert need > 0
    out, scratch = _guarded(4 * h * w, fill), _guarded(need, fill)
    md = dev(np.array(m).reshape(-1))                                                # (a copy: the shared inputs are read-only)
    vd = None if veil is None else dev(np.array(veil).reshape(-1))
    _lib.call("drs_distance_transform", md.data_ptr(), None if vd is None else vd.data_ptr(), 0 if veil_label is None else veil_label,
              h, w, mode, cls, out.data_ptr(), scratch.data_ptr(), need, stream())
    torch.cuda.synchronize()
    assert _guard_ok(out, 4 * h * w, fill) and _guard_ok(scratch, need, fill), "a guard region was written"
    return out[:4 * h * w].cpu().numpy().view(np.uint32).reshape(h, w).astype(np.int64)


def _table(truth, pred, K, ignore, table=None, fill=0xA5):
    from drs_amd import _lib
    h, w = truth.shape
    need = _lib.query("drs_surface_scratch_bytes", h, w)
    assert need > 0
    scratch = _guarded(need, fill)
    table = torch.zeros(2 * K * (BINS + 2), dtype=torch.int64, device=DEV) if table is None else table
    t, p = dev(np.array(truth).reshape(-1)), dev(np.array(pred).reshape(-1))
    _lib.call("drs_surface_histogram", t.data_ptr(), p.data_ptr(), h, w, K, ignore, table.data_ptr(), scratch.data_ptr(), need, stream())
    torch.cuda.synchronize()
    assert _guard_ok(scratch, need, fill), "the guard region behind the scratch was written"
    return table.cpu().numpy().reshape(2, K, BINS + 2)


# ------------------------------------------------------------------------------------------------------------- 1. the transform
def _sparse(h, w, count, seed):
    """zeros with `count` seeded single pixels of byte 1: the same sites in all three modes (CLASS 1, CONTOUR 1, NOT_CLASS 0)"""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), dtype=np.uint8)
    m[rng.integers(0, h, count), rng.integers(0, w, count)] = 1
    return m


def _corner():
    m = np.zeros((130, 67), dtype=np.uint8)
    m[0, 0] = 1
    return m


def _row_and_column():
    m = np.zeros((70, 90), dtype=np.uint8)
    m[:, 23] = 2                                                                     # a class that fills exactly one column
    m[17, :] = 1                                                                     # ... and one that fills exactly one row
    return m


def _checkerboard():
    yy, xx = np.mgrid[0:33, 0:37]
    return ((yy + xx) & 1).astype(np.uint8)


ALL = lambda cls: [(R.CLASS, cls), (R.NOT_CLASS, cls), (R.CONTOUR, cls)]
SPARSE = [(R.CLASS, 1), (R.CONTOUR, 1), (R.NOT_CLASS, 0)]
# id -> (the map, the (mode, cls) pairs, veil, veil_label)
TRANSFORMS = {
    "45x131": (lambda: R.synthetic_case(45, 131, 6, seed=0, ignore=6)[1], ALL(1) + ALL(0), None, None),
    "5x7": (lambda: R.synthetic_case(5, 7, 2, seed=0)[1], ALL(0) + ALL(1), None, None),
    "1x40": (lambda: R.synthetic_case(1, 40, 3, seed=0)[1], ALL(0) + ALL(1), None, None),
    "40x1": (lambda: R.synthetic_case(40, 1, 3, seed=0)[1], ALL(0) + ALL(1), None, None),
    "64x64-uniform": (lambda: np.full((64, 64), 2, dtype=np.uint8), [(R.CLASS, 3), (R.NOT_CLASS, 2), (R.CONTOUR, 2), (R.CLASS, 2)], None, None),
    "130x67-corner": (_corner, SPARSE, None, None),
    "row-and-column": (_row_and_column, ALL(1) + ALL(2) + ALL(0), None, None),
    "checkerboard": (_checkerboard, ALL(0) + ALL(1), None, None),
    "63x65": (lambda: _sparse(TILE - 1, TILE + 1, 30, 1), SPARSE, None, None),
    "65x63": (lambda: _sparse(TILE + 1, TILE - 1, 30, 2), SPARSE, None, None),
    "15x257": (lambda: R.synthetic_case(ROWS - 1, WIDE + 1, 3, seed=5)[1], ALL(0) + ALL(1), None, None),
    "17x255": (lambda: R.synthetic_case(ROWS + 1, WIDE - 1, 3, seed=6)[1], ALL(0) + ALL(1), None, None),
    "300x517-sparse": (lambda: _sparse(300, 517, 40, 3), SPARSE, None, None),
    "45x131-veil": (lambda: R.synthetic_case(45, 131, 6, seed=0, ignore=6)[1], ALL(6) + ALL(1), "truth", 6),
}
_MAPS = {}


def _map(name):
    if name not in _MAPS:
        make, pairs, veil, veil_label = TRANSFORMS[name]
        m = make()
        v = R.synthetic_case(45, 131, 6, seed=0, ignore=6)[0] if veil == "truth" else None
        for a in (m, v):
            if a is not None:
                a.setflags(write=False)
        _MAPS[name] = (m, v)
    return _MAPS[name]


@pytest.mark.parametrize("name", sorted(TRANSFORMS))
def test_transform(name):
    m, veil = _map(name)
    _, pairs, _, veil_label = TRANSFORMS[name]
    for mode, cls in pairs:
        want = R.distance2(m, mode, cls, veil, veil_label)
        np.testing.assert_array_equal(_transform(m, mode, cls, veil, veil_label), want, err_msg="mode %d cls %d" % (mode, cls))
    if name == "64x64-uniform":
        assert all((R.distance2(m, mode, cls) == INF).all() for mode, cls in pairs[:3]) and (R.distance2(m, *pairs[3]) == 0).all()
    if name == "130x67-corner":
        assert R.distance2(m, R.CLASS, 1)[129, 66] == 129 * 129 + 66 * 66
    if name == "checkerboard":
        assert R.sites(m, R.CONTOUR, 0).sum() + R.sites(m, R.CONTOUR, 1).sum() == m.size
    if name == "45x131-veil":
        assert (R.sites(m, R.CLASS, 6, veil, 6) != R.sites(m, R.CLASS, 6)).any()     # the veil changes the sites


def test_transform_does_not_read_what_it_did_not_write_and_repeats_its_bits():
    m, veil = _map("45x131-veil")
    for mode, cls in ((R.CONTOUR, 1), (R.NOT_CLASS, 6)):
        poisoned = _transform(m, mode, cls, veil, 6, fill=0xA5)
        np.testing.assert_array_equal(poisoned, _transform(m, mode, cls, veil, 6, fill=0x00))
        np.testing.assert_array_equal(poisoned, _transform(m, mode, cls, veil, 6, fill=0xA5))
    empty = np.full((64, 64), 2, dtype=np.uint8)
    assert (_transform(empty, R.CLASS, 3, fill=0x00) == INF).all()


def test_loops_distance_transform_is_a_thin_call():
    from drs_amd import loops
    m, veil = _map("45x131-veil")
    md, vd = dev(np.array(m)), dev(np.array(veil))
    got = loops.distance_transform(md, 45, 131, "contour", 1)
    assert got.dtype == torch.int32 and tuple(got.shape) == (45, 131) and got.device == md.device
    np.testing.assert_array_equal(got.cpu().numpy(), R.distance2(m, R.CONTOUR, 1))
    got = loops.distance_transform(md.reshape(-1), 45, 131, R.NOT_CLASS, 6, veil=vd, veil_label=6, stream=stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), R.distance2(m, R.NOT_CLASS, 6, veil, 6))
    assert (loops.distance_transform(md, 45, 131, "class", 77).cpu().numpy() == INF).all()
    for kw, say in ((dict(mode=3), "mode"), (dict(mode="edge"), "mode"), (dict(veil=vd), "go together"), (dict(h=44), "44 x 131")):
        a = dict(dict(map_dev=md, h=45, w=131, mode=0, cls=1), **kw)
        with pytest.raises(ValueError, match=say):
            loops.distance_transform(**a)


# ------------------------------------------------------------------------------------------------------------- 2. the table
def _absent():
    truth, pred = R.synthetic_case(45, 131, 6, seed=2)
    pred = pred.copy()
    pred[pred == 1] = 0                                                              # class 1 is in the truth and not in the prediction
    return truth, pred


def _far():
    truth, pred = np.zeros((2, 1100), dtype=np.uint8), np.zeros((2, 1100), dtype=np.uint8)
    truth[:, 0:2] = 1
    pred[:, 1098:1100] = 1
    return truth, pred


def _bytes_above_K():
    truth, pred = R.synthetic_case(33, 65, 2, seed=1)
    pred = pred.copy()
    pred[10:12, 5:40] = 200                                                          # a bar of a byte >= K: it draws contours, it has no row
    return truth, pred


# id -> (the pair, K, ignore)
TABLES = {
    "K6-ignore6": (lambda: R.synthetic_case(45, 131, 6, seed=0, ignore=6), 6, 6),
    "K2": (_bytes_above_K, 2, -1),
    "K8-ignore7": (lambda: R.synthetic_case(40, 70, 8, seed=4, ignore=7), 8, 7),
    "absent-class": (_absent, 6, -1),
    "2x1100-far": (_far, 2, -1),
}
_PAIRS = {}


def _pair(name):
    """the two maps and the reference table of a case, computed once and shared by the tests (read-only)"""
    if name not in _PAIRS:
        make, K, ignore = TABLES[name]
        truth, pred = make()
        want = R.table(truth, pred, K, ignore)
        for a in (truth, pred, want):
            a.setflags(write=False)
        _PAIRS[name] = (truth, pred, want)
    return _PAIRS[name]


@pytest.mark.parametrize("name", sorted(TABLES))
def test_table(name):
    _, K, ignore = TABLES[name]
    truth, pred, want = _pair(name)
    got = _table(truth, pred, K, ignore)
    np.testing.assert_array_equal(got, want)
    for c in range(K):                                                               # a row's bins hold the contour set, pixel for pixel
        st, sp = R.contour_sets(truth, pred, c, ignore)
        sizes = (0, 0) if c == ignore else (int(st.sum()), int(sp.sum()))
        assert (int(got[0, c, :BINS].sum() + got[0, c, BINS + 1]), int(got[1, c, :BINS].sum() + got[1, c, BINS + 1])) == sizes, c
    if name == "K6-ignore6":
        assert (got[:, :, :BINS].sum(axis=2) > 0).all(axis=0).sum() >= 4           # four classes with a contour in both maps
    if name == "K8-ignore7":
        assert got[:, 7].sum() == 0 and (np.asarray(truth) == 7).any()
    if name == "absent-class":
        assert got[0, 1, BINS + 1] > 0 and got[0, 1, :BINS + 1].sum() == 0 and got[1, 1].sum() == 0
    if name == "2x1100-far":
        assert got[0, 1, BINS - 1] == 2 == got[1, 1, BINS - 1] and got[0, 1, BINS] == 2 * 1097 * 1024


def test_counters_are_added_to_and_two_runs_give_the_same_bits():
    _, K, ignore = TABLES["K6-ignore6"]
    truth, pred, want = _pair("K6-ignore6")
    rng = np.random.default_rng(1)
    before = rng.integers(1, 1 << 40, size=(2, K, BINS + 2), dtype=np.int64)
    table = dev(before.reshape(-1))
    _table(truth, pred, K, ignore, table)
    got = _table(truth, pred, K, ignore, table)
    np.testing.assert_array_equal(got, before + 2 * want)
    np.testing.assert_array_equal(_table(truth, pred, K, ignore, fill=0x00), _table(truth, pred, K, ignore, fill=0xA5))


def test_loops_surface_histogram_is_a_thin_call():
    from drs_amd import loops
    _, K, ignore = TABLES["K6-ignore6"]
    truth, pred, want = _pair("K6-ignore6")
    t, p = dev(np.array(truth).reshape(-1)), dev(np.array(pred))
    table = loops.surface_histogram(t, p, 45, 131, K, ignore)
    assert table.dtype == torch.int64 and tuple(table.shape) == (2, K, BINS + 2) and table.device == t.device
    again = loops.surface_histogram(t, p, 45, 131, K, ignore, table=table, stream=stream())
    torch.cuda.synchronize()
    assert again is table
    np.testing.assert_array_equal(table.cpu().numpy(), 2 * want)
    none = loops.surface_histogram(t, p, 45, 131, K, None).cpu().numpy()
    np.testing.assert_array_equal(none, R.table(truth, pred, K, -1))
    with pytest.raises(ValueError, match="int64"):
        loops.surface_histogram(t, p, 45, 131, K, ignore, table=torch.zeros(2 * K * (BINS + 2), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="uint8"):
        loops.surface_histogram(t.to(torch.int32), p, 45, 131, K, ignore)


# ------------------------------------------------------------------------------------------------------------- 3. arguments
def test_rejected_arguments_return_err_arg_and_launch_nothing():
    from drs_amd import _lib
    h, w, K, ignore = 5, 7, 2, -1
    truth, pred = R.synthetic_case(h, w, K, seed=0)
    t, p = dev(truth.reshape(-1)), dev(pred.reshape(-1))
    table = torch.full((2 * K * (BINS + 2),), 7, dtype=torch.int64, device=DEV)
    d2 = torch.full((h * w,), 77, dtype=torch.int32, device=DEV)
    nd, ns = _lib.query("drs_distance_scratch_bytes", h, w), _lib.query("drs_surface_scratch_bytes", h, w)
    scratch = torch.full((max(nd, ns),), 0x5A, dtype=torch.uint8, device=DEV)
    good = dict(map=t.data_ptr(), veil=p.data_ptr(), veil_label=1, h=h, w=w, mode=2, cls=1, d2=d2.data_ptr(), scratch=scratch.data_ptr(), n=nd)
    for kw in (dict(map=None), dict(d2=None), dict(scratch=None), dict(h=0), dict(w=0), dict(h=32769), dict(h=32768, w=16384), dict(mode=-1),
               dict(mode=3), dict(cls=-1), dict(cls=256), dict(veil_label=-1), dict(veil_label=256), dict(n=nd - 1)):
        a = dict(good, **kw)
        assert _lib.query("drs_distance_transform", *[a[k] for k in good], stream()) == 1, kw
    good = dict(truth=t.data_ptr(), pred=p.data_ptr(), h=h, w=w, K=K, ignore=ignore, table=table.data_ptr(), scratch=scratch.data_ptr(), n=ns)
    for kw in (dict(truth=None), dict(pred=None), dict(table=None), dict(scratch=None), dict(h=0), dict(w=-1), dict(w=32769), dict(K=1),
               dict(K=9), dict(ignore=-2), dict(ignore=256), dict(n=ns - 1)):
        a = dict(good, **kw)
        assert _lib.query("drs_surface_histogram", *[a[k] for k in good], stream()) == 1, kw
    torch.cuda.synchronize()
    assert (table == 7).all() and (d2 == 77).all() and (scratch == 0x5A).all()       # nothing was launched
    assert _lib.query("drs_surface_histogram", *[good[k] for k in good], stream()) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(table.cpu().numpy().reshape(2, K, BINS + 2), 7 + R.table(truth, pred, K, ignore))


# ------------------------------------------------------------------------------------------------------------- 4. the loop
CH, K6 = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
TOL = (1, 2, 4)


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


def _same_scores(got, want):
    assert set(want) <= set(got)
    for key, v in want.items():
        np.testing.assert_array_equal(np.asarray(got[key], dtype=np.float64), np.asarray(v, dtype=np.float64), err_msg=key)


def test_validate_test_reports_the_tables_of_the_maps_it_scored(capsys):
    from drs_amd import loops, metrics as MT
    from drs_amd.synthetic import make_tile
    tiles, labs = zip(*[make_tile(h, w, CH, K6, seed=s, n_seeds=30) for h, w, s in ((44, 50, 21), (37, 61, 22))])
    tiles, labs = list(tiles), list(labs)
    d = _net()
    capsys.readouterr()
    res0 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7)
    text0 = capsys.readouterr().out
    res_none = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, surface_scores=None)
    # (None is "no option": the same text and a pair, not a triple.  That nothing else moved is what the comparison of every
    # non-Surface line of the option-on run below shows; neither can see a difference from an earlier commit)
    assert capsys.readouterr().out == text0 and len(res_none) == len(res0) == 2
    cm1, maps1, extra = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, surface_scores=TOL)
    text1 = capsys.readouterr().out
    np.testing.assert_array_equal(res0[0], cm1)
    np.testing.assert_array_equal(res0[0], res_none[0])
    for m0, m1, m2 in zip(res0[1], maps1, res_none[1]):
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(m0, m2)
    assert set(extra) == {"surface"}
    s = extra["surface"]
    per_map = [R.table(lab, m, K6, 6) for lab, m in zip(labs, maps1)]
    assert s["table"].dtype == np.int64 and s["table"].shape == (2, K6, BINS + 2) and s["tolerances"] == TOL
    np.testing.assert_array_equal(s["table"], per_map[0] + per_map[1])
    _same_scores(s, MT.surface_scores(per_map[0] + per_map[1], TOL))
    assert len(s["per_map"]) == 2
    for got, table in zip(s["per_map"], per_map):
        np.testing.assert_array_equal(got["table"], table)
        _same_scores(got, MT.surface_scores(table, TOL))
    assert s["n_truth"].sum() > 0 and s["n_pred"].sum() > 0
    # the Surface lines: one per map after the map's reference-format line, one for all maps; everything else byte for byte
    lines0, lines1 = text0.splitlines(), text1.splitlines()
    mine = [i for i, line in enumerate(lines1) if ": Surface tau= 1 2 4 Truth Contour= [" in line]
    assert len(mine) == 3 and lines0
    assert [line for i, line in enumerate(lines1) if i not in mine] == lines0
    for i, who in zip(mine, ("Test Map a: ", "Test Map b: ", "Test ALL MAPS: ")):
        assert lines1[i].startswith("---- Iter 7 -- " + who + "Surface tau= ")
        assert lines1[i - 1].startswith("---- Iter 7 -- " + who + "Overall Accuracy= ")
    assert lines1[mine[-1]] == "---- Iter 7 -- Test ALL MAPS: " + loops._surface_str(s)
    # beside the other score options the keys of all reports are there, and the Surface line is the map's last
    _, sieved, both = loops.validate_test(d, tiles[:1], labs[:1], ["a"], 6, MEAN, STD, 25, 7, surface_scores=TOL, boundary_scores=(1, 2),
                                          object_scores=4, sieve=4)
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("---- Iter 7 -- Test ")]
    assert {"surface", "boundary", "objects", "sieve"} == set(both)
    assert [": Surface tau=" in x for x in lines] == [False, False, False, False, True] * 2
    # ... and it is the sieved map, the one drs_confusion scored, that the table describes
    np.testing.assert_array_equal(both["surface"]["table"], R.table(labs[0], sieved[0], K6, 6))
