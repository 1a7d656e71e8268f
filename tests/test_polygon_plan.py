"""The polygon output without a device: the numpy statement tests/polygon_ref.py against its own lemmas and known
answers, the host side (vectors.polygons_of / geojson / write_geojson), the option's values (patches.check_polygons), the command
line, and the argument checks of the four entry points (include/drs.h drs_polygon_count / drs_polygon_scratch_bytes /
drs_polygon_rings / drs_polygon_write).  Every comparison is exact."""
import ctypes as C
import json

import numpy as np
import pytest

import polygon_ref as R
import sieve_ref
from drs_amd import patches as P

MAPS = {
    "speckled-45x131-K6": lambda: sieve_ref.speckled(45, 131, 6),
    "serpentine-67x131": lambda: sieve_ref.serpentine(67, 131),
    "checkerboard-67x131": lambda: sieve_ref.checkerboard(67, 131),
    "uniform-300x300": lambda: sieve_ref.uniform(300, 300),
}
_CACHE = {}


def _case(name, c):
    """(map, label, size, ring table, vertices) of the reference, computed once (read-only)"""
    if (name, c) not in _CACHE:
        m = MAPS[name]()
        label, size = sieve_ref.components(m, c)
        _CACHE[name, c] = (m, label, size) + R.rings(m, c, label=label)
        for a in _CACHE[name, c]:
            a.setflags(write=False)
    return _CACHE[name, c]


CASES = [(n, c) for n in MAPS for c in (4, 8)]


# ------------------------------------------------------------------------------------------------------------- the reference's lemmas
@pytest.mark.parametrize("name, c", CASES)
def test_ref_succ_is_a_bijection_that_joins_head_to_tail(name, c):
    m = _case(name, c)[0]
    w = m.shape[1]
    ids = R.cracks(m)
    nxt = R.succ(m, ids, c)
    np.testing.assert_array_equal(np.sort(nxt), ids)
    head = lambda e: ((e >> 2) % w + R.HX[e & 3], (e >> 2) // w + R.HY[e & 3])
    tail = lambda e: ((e >> 2) % w + R.HX[(e & 3) - 1], (e >> 2) // w + R.HY[(e & 3) - 1])
    for a, b in zip(head(ids), tail(nxt)):
        np.testing.assert_array_equal(a, b)
    assert R.succ(m, int(ids[0]), c) == nxt[0]                                      # one id as well as many


@pytest.mark.parametrize("name, c", CASES)
def test_ref_rings_tile_the_map(name, c):
    m, label, size, table, verts = _case(name, c)
    h, w = m.shape
    assert table[:, 6].sum() == 2 * h * w and (table[:, 6] != 0).all()
    assert (np.diff(table[:, 0]) > 0).all() and table[:, 5].sum() == len(R.cracks(m)) and table[:, 4].sum() == len(verts)
    np.testing.assert_array_equal(table[:, 3], np.cumsum(table[:, 4]) - table[:, 4])
    assert (table[:, 4] % 2 == 0).all() and (table[:, 4] >= 4).all()
    np.testing.assert_array_equal(table[:, 1], label.reshape(-1)[table[:, 0] >> 2])  # a cycle stays inside one component
    np.testing.assert_array_equal(table[:, 2], m.reshape(-1)[table[:, 0] >> 2])
    # per label one positive ring, whose id is 4 label, and the areas add up to the component's size
    roots = np.unique(label)
    pos = table[table[:, 6] > 0]
    np.testing.assert_array_equal(pos[:, 1], roots)
    np.testing.assert_array_equal(pos[:, 0], 4 * roots)
    area = np.zeros(h * w, dtype=np.int64)
    np.add.at(area, table[:, 1], table[:, 6])
    np.testing.assert_array_equal(area[roots], 2 * size.reshape(-1)[roots].astype(np.int64))


@pytest.mark.parametrize("name, c", CASES)
def test_ref_fill_gives_back_the_components(name, c):
    m, label, _, table, verts = _case(name, c)
    h, w = m.shape
    rings = R.ring_vertices(table, verts)
    roots = np.unique(label)
    for root in (roots if len(roots) <= 40 else roots[:: len(roots) // 40]):
        mine = [r for r, row in zip(rings, table) if row[1] == root]
        np.testing.assert_array_equal(R.fill(h, w, mine), label == root)
    # all rings of one byte at once: the even-odd rule cancels what a hole's island puts back
    for b in np.unique(m):
        np.testing.assert_array_equal(R.fill(h, w, [r for r, row in zip(rings, table) if row[2] == b]), m == b)


# (map, c) -> cracks, rings, vertices, longest ring, holes; None = not recorded
KNOWN = {("speckled-45x131-K6", 4): (6488, 1070, 5652, 452, 340), ("speckled-45x131-K6", 8): (6488, 1186, 5652, None, None),
         ("serpentine-67x131", 4): (17622, 34, 268, 8976, None), ("serpentine-67x131", 8): (17622, 34, 268, 8976, None),
         ("checkerboard-67x131", 4): (35108, 8777, None, None, None), ("checkerboard-67x131", 8): (35108, 8387, None, None, 8385),
         ("uniform-300x300", 4): (1200, 1, 4, None, None), ("uniform-300x300", 8): (1200, 1, 4, None, None)}


@pytest.mark.parametrize("name, c", CASES)
def test_ref_known_answers(name, c):
    m, _, _, table, verts = _case(name, c)
    got = (len(R.cracks(m)), len(table), len(verts), int(table[:, 5].max()), int((table[:, 6] < 0).sum()))
    for g, want in zip(got, KNOWN[name, c]):
        assert want is None or g == want, (got, KNOWN[name, c])


def test_ref_a_pinch_and_a_diagonal_hole():
    """two diagonal pixels: two rings at 4, one ring that touches itself at 8; a hole between diagonal pixels at 4"""
    m = np.array([[1, 0], [0, 1]], dtype=np.uint8)
    t4, v4 = R.rings(m, 4)
    assert len(t4) == 4 and (t4[:, 4] == 4).all() and (t4[:, 6] == 2).all()
    t8, v8 = R.rings(m, 8)
    assert t8[:, [0, 4, 5, 6]].tolist() == [[0, 8, 8, 4], [4, 8, 8, 4]]
    assert v8[:8].tolist() == [[1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1], [0, 0]]
    m = np.ones((4, 4), dtype=np.uint8)
    m[1, 1] = m[2, 2] = 0
    t4, _ = R.rings(m, 4)
    assert sorted(t4[:, 6].tolist()) == [-4, 2, 2, 32] and t4[t4[:, 6] == -4][0, 4] == 8           # one hole around both, pinched
    t8, _ = R.rings(m, 8)
    assert sorted(t8[:, 6].tolist()) == [-2, -2, 4, 32]


# ------------------------------------------------------------------------------------------------------------- the host side
# byte 9 frames byte 1, which has a hole of byte 2, in which lies an island of byte 1
HAND = np.array([[9, 9, 9, 9, 9, 9, 9],
                 [9, 1, 1, 1, 1, 1, 9],
                 [9, 1, 2, 2, 2, 1, 9],
                 [9, 1, 2, 1, 2, 1, 9],
                 [9, 1, 2, 2, 2, 1, 9],
                 [9, 1, 1, 1, 1, 1, 9],
                 [9, 9, 9, 9, 9, 9, 9]], dtype=np.uint8)


def _shoelace(ring):
    r = np.asarray(ring, dtype=np.float64)
    return float((r[:-1, 0] * r[1:, 1] - r[1:, 0] * r[:-1, 1]).sum())


def test_vectors_group_close_and_describe():
    from drs_amd import vectors
    table, verts = R.rings(HAND, 4)
    groups = vectors.polygons_of(table, verts)
    assert [(b, lab, len(ext), [len(h) for h in holes]) for b, lab, ext, holes in groups] == [
        (9, 0, 4, [4]), (1, 8, 4, [4]), (2, 16, 4, [4]), (1, 24, 4, [])]
    doc = vectors.geojson(table, verts, 3, class_names=["a", "b", "c"])
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == 3                      # byte 9 >= K is skipped
    props = [f["properties"] for f in doc["features"]]
    assert props == [dict([("class", 1), ("class_name", "b"), ("component", 8), ("pixels", 16), ("perimeter", 32)]),
                     dict([("class", 2), ("class_name", "c"), ("component", 16), ("pixels", 8), ("perimeter", 16)]),
                     dict([("class", 1), ("class_name", "b"), ("component", 24), ("pixels", 1), ("perimeter", 4)])]
    assert list(props[0]) == ["class", "class_name", "component", "pixels", "perimeter"]
    assert "class_name" not in vectors.geojson(table, verts, 3)["features"][0]["properties"]
    for f in doc["features"]:
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon"
        rings = f["geometry"]["coordinates"]
        for k, ring in enumerate(rings):
            assert ring[0] == ring[-1] and all(isinstance(v, int) for pt in ring for v in pt)
            assert (_shoelace(ring) > 0) == (k == 0)                                                # exterior first, then the holes
        assert sum(_shoelace(r) for r in rings) == 2 * f["properties"]["pixels"]
    assert doc["features"][0]["geometry"]["coordinates"][0] == [[6, 1], [6, 6], [1, 6], [1, 1], [6, 1]]
    assert len(vectors.geojson(table, verts, 10)["features"]) == 4 and vectors.geojson(table, verts, 1)["features"] == []


@pytest.mark.parametrize("transform, reversed_", [((1, 0, 0, 0, 1, 0), False), ((0.5, 0, 100, 0, -0.5, 900), True), ((0, 1, 0, 1, 0, 0), True),
                                                   ((-2, 0, 5, 0, -2, 7), False), ((0, -1, 3, 1, 0, 4), False)])
def test_vectors_reverse_exactly_when_the_transform_mirrors(transform, reversed_):
    from drs_amd import vectors
    table, verts = R.rings(HAND, 4)
    plain = vectors.geojson(table, verts, 3)["features"]
    a, b, c, d, e, f = transform
    for got, ref in zip(vectors.geojson(table, verts, 3, transform=transform)["features"], plain):
        assert got["properties"] == ref["properties"]
        for k, (ring, src) in enumerate(zip(got["geometry"]["coordinates"], ref["geometry"]["coordinates"])):
            want = [[float(a * x + b * y + c), float(d * x + e * y + f)] for x, y in src]
            assert ring == (want[::-1] if reversed_ else want) and all(isinstance(v, float) for pt in ring for v in pt)
            assert (_shoelace(ring) > 0) == (k == 0)                                                # RFC 7946 whatever the transform


def test_vectors_refuse_a_tampered_table(tmp_path):
    from drs_amd import vectors
    table, verts = R.rings(HAND, 4)
    bad = table.copy()
    hole = np.nonzero((bad[:, 1] == 8) & (bad[:, 6] < 0))[0][0]
    bad[hole, 6] = -bad[hole, 6]                                                                   # two positive rings of label 8
    with pytest.raises(ValueError, match="component 8: 2 rings of positive area"):
        vectors.polygons_of(bad, verts)
    with pytest.raises(ValueError, match="component 8"):
        vectors.geojson(bad, verts, 3)
    bad = table.copy()
    bad[0, 6] = -bad[0, 6]                                                                         # none
    with pytest.raises(ValueError, match="component 0: 0 rings of positive area"):
        vectors.polygons_of(bad, verts)
    with pytest.raises(ValueError, match="lie outside"):
        vectors.polygons_of(table, verts[:-1])
    with pytest.raises(ValueError, match="6 numbers"):
        vectors.geojson(table, verts, 3, transform=(1, 0, 0, 1))
    path = tmp_path / "hand.geojson"
    doc = vectors.write_geojson(str(path), table, verts, 3)
    text = path.read_text()
    assert json.loads(text) == doc and "." not in text                                             # integers stay integers


# ------------------------------------------------------------------------------------------------------------- the option and the CLI
def test_check_polygons():
    assert P.check_polygons(4) == 4 and P.check_polygons(np.int64(8)) == 8 and P.POLYGON_CONNECTIVITY == 4
    for bad in (6, 0, True, "4", 4.0, None, (4,)):
        with pytest.raises(ValueError, match="expected 4 or 8"):
            P.check_polygons(bad)
    assert P.parse_polygons("8") == 8
    for bad in ("", "6", " 4", "4,8", 4):
        with pytest.raises(ValueError):
            P.parse_polygons(bad)


ARGV = ["x.py", "a", "b"]
MAIN_ARGV = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
             "single_fixed", "25", "acc"]


def test_cli_parse_polygons_anywhere_in_argv():
    from drs_amd import cli
    got, value = cli.parse_polygons(ARGV)
    assert value is None and got == ARGV and got is not ARGV
    assert cli.parse_polygons(["--polygons"] + ARGV) == (ARGV, 4)
    assert cli.parse_polygons(["x.py", "a", "--polygons=8", "b"]) == (ARGV, 8)
    # the bare flag follows the sieve's connectivity; a value of its own does not
    assert cli.parse_polygons(ARGV + ["--polygons"], P.check_sieve(dict(min_size=9, connectivity=8))) == (ARGV, 8)
    assert cli.parse_polygons(ARGV + ["--polygons"], P.check_sieve(9)) == (ARGV, 4)
    assert cli.parse_polygons(ARGV + ["--polygons=4"], P.check_sieve(dict(min_size=9, connectivity=8))) == (ARGV, 4)
    for bad, say in ((["--polygons="], "--polygons=: expected --polygons or --polygons=4|8"), (["--polygons=6"], "--polygons=6: expected"),
                     (["--polygons", "--polygons=8"], "more than once"), (["--polygons=8", "--polygons=8"], "more than once")):
        with pytest.raises(ValueError) as e:
            cli.parse_polygons(ARGV + bad)
        assert say in str(e.value), (bad, str(e.value))


def test_cli_flag_outside_generate_final_maps_exits():
    from drs_amd import cli
    from drs_amd.net import NoComm
    for tail, say in ((["training", "--polygons"], "--polygons applies to the generate_final_maps process only"),
                      (["validate_test", "--polygons=8"], "--polygons applies to the generate_final_maps process only"),
                      (["generate_final_maps", "--polygons=5"], "--polygons=5: expected"),
                      (["generate_final_maps", "--polygons", "--polygons"], "more than once")):
        with pytest.raises(SystemExit) as e:
            cli.main(MAIN_ARGV + tail, device="cpu", comm=NoComm())
        assert say in str(e.value), (tail, str(e.value))
    assert "--polygons[=4|8]" in cli.__doc__


class _Reached(Exception):
    pass


@pytest.mark.parametrize("flags, want", [([], "absent"), (["--polygons"], 4), (["--polygons=8"], 8),
                                         (["--polygons", "--sieve=9", "--sieve-connectivity=8"], 8),
                                         (["--sieve-connectivity=8", "--polygons=4", "--sieve=9", "--crf"], 4)])
def test_cli_flag_reaches_the_loop(monkeypatch, tmp_path, flags, want):
    """main parses, loads the synthetic tiles and calls the loop with polygons=...: the net and the checkpoint are stand-ins, the loop
    itself is intercepted.  Without the flag the loop is called without the argument at all."""
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
    monkeypatch.setattr(loops, "generate_final_maps", loop)
    argv = list(MAIN_ARGV)
    argv[1], argv[2], argv[3] = "synthetic:30x32x5/vaihingen/", str(tmp_path) + "/", "model-7"
    with pytest.raises(_Reached):
        cli.main(argv + ["generate_final_maps"] + flags, device="cpu", comm=NoComm())
    assert seen.get("polygons", "absent") == want
    assert ("crf" in seen) == ("--crf" in flags) and ("sieve" in seen) == ("--sieve=9" in flags)


def test_the_loops_refuse_a_bad_value_before_they_touch_the_net():
    from drs_amd import loops
    with pytest.raises(ValueError, match="connectivity 6"):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, polygons=6)
    with pytest.raises(ValueError, match="connectivity True"):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, polygons=True)


def test_polygons_str():
    from drs_amd import loops
    table, _ = R.rings(HAND, 4)
    info = loops._polygons_info(table, {"cracks": 80}, 3)
    assert info == {"per_class": [0, 2, 1], "holes": 2, "vertices": 20, "cracks": 80}
    assert loops._polygons_str(4, info) == "Polygons connectivity= 4 Polygons per class= [0 2 1] Holes= 2 Vertices= 20"
    assert loops._polygons_str(8, [info, info]) == "Polygons connectivity= 8 Polygons per class= [0 4 2] Holes= 4 Vertices= 40"


# ------------------------------------------------------------------------------------------------------------- the entry points
def test_entry_points_reject_what_is_outside_their_ranges():
    """Ranges, else DRS_ERR_ARG: checked on the host before anything is launched or read, so no device is needed.  The pointers are
    small integers no call may follow."""
    from drs_amd import _lib
    lib = _lib.load()
    ok = dict(map=8, label=16, h=5, w=7, c=4, cap=140, scratch=24, counters=32)
    order = ("map", "label", "h", "w", "c", "cap", "scratch", "counters")
    for kw in (dict(map=None), dict(label=None), dict(scratch=None), dict(counters=None), dict(h=0), dict(w=0), dict(h=-5), dict(h=1 << 14, w=(1 << 14) + 1),
               dict(c=0), dict(c=6), dict(c=-4), dict(cap=0), dict(cap=141), dict(cap=-1)):
        a = dict(ok, **kw)
        assert lib.drs_polygon_rings(*[a[k] for k in order], None) == 1, kw
    for args in ((None, 5, 7, 8), (8, 5, 7, None), (8, 0, 7, 16), (8, 5, 0, 16), (8, 1 << 14, (1 << 14) + 1, 16)):
        assert lib.drs_polygon_count(*args, None) == 1, args
    okw = dict(scratch=8, h=5, w=7, cap=140, ring_cap=3, vertex_cap=9, table=16, vertices=24, status=32)
    for kw in (dict(scratch=None), dict(table=None), dict(vertices=None), dict(status=None), dict(h=0), dict(w=-1), dict(h=1 << 14, w=(1 << 14) + 1),
               dict(cap=0), dict(cap=141), dict(ring_cap=-1), dict(vertex_cap=-1)):
        a = dict(okw, **kw)
        assert lib.drs_polygon_write(*[a[k] for k in okw], None) == 1, kw
    q = lib.drs_polygon_scratch_bytes
    assert q(0, 7, 4) == 0 == q(5, 0, 4) == q(5, 7, 0) == q(5, 7, 141) == q(1 << 14, (1 << 14) + 1, 4) == q(5, 7, -1)
    assert q(5, 7, 140) > q(5, 7, 4) > 0 and q(1 << 14, 1 << 14, 1 << 30) > 66 << 30
    assert isinstance(C.c_size_t(q(5, 7, 4)).value, int)
