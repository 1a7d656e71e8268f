"""-m gpu: the polygon outlines of a label map (include/drs.h drs_polygon_count / drs_polygon_rings /
drs_polygon_write; loops.polygons, generate_final_maps' polygons) against their numpy statement tests/polygon_ref.py.

Every comparison is exact integer equality: the rule is integer arithmetic, there are no tolerances and no excluded elements."""
import json
import os

import numpy as np
import pytest
import torch

import polygon_ref as R
import sieve_ref

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402


def _stripes(h, w):
    """vertical stripes two pixels wide, bytes 0 and 1: about one crack per pixel, every stripe one component at 4 and at 8"""
    return np.broadcast_to(((np.arange(w) >> 1) & 1).astype(np.uint8), (h, w)).copy()


# the smallest maps at which each part can go wrong: ragged with many rings, holes and pinches; one-pixel-wide maps; one pixel; one ring
# of 4 vertices and 1200 collinear cracks; a ring of 8976 cracks (the doubling's depth); cracks = 4 h w - ..., 8385 holes at 8; nested
# rings; noise.  The scans work on blocks of 1024 elements, a second level from 1025 elements and a third from 1024^2 + 1:
# stripes-1025x1024 has 1 049 600 pixels and 1 051 648 cracks, so that BOTH scans -- the per-pixel crack counts and the ring leaders
# over the crack slots -- run all three levels, with a last block that is not full at every level (1025 and 1027 blocks, then 2).
# The other maps cover one level (up to 1024 elements: 1x1, 5x7, 1x40, 40x1) and two.
MAPS = {
    "speckled-45x131-K6": lambda: sieve_ref.speckled(45, 131, 6),
    "speckled-1x40": lambda: sieve_ref.speckled(1, 40, 3),
    "speckled-40x1": lambda: sieve_ref.speckled(40, 1, 3),
    "speckled-5x7": lambda: sieve_ref.speckled(5, 7, 2),
    "one-1x1": lambda: np.full((1, 1), 3, dtype=np.uint8),
    "uniform-64x64": lambda: sieve_ref.uniform(64, 64),
    "uniform-300x300": lambda: sieve_ref.uniform(300, 300),
    "serpentine-67x131": lambda: sieve_ref.serpentine(67, 131),
    "checkerboard-67x131": lambda: sieve_ref.checkerboard(67, 131),
    "rings": lambda: sieve_ref.rings(),
    "noise-64x64-K4": lambda: sieve_ref.noise(),
    "stripes-1025x1024": lambda: _stripes(1025, 1024),
}
CASES = [(n, c) for n in MAPS for c in (4, 8)]
SENTINEL = -0x0123456789ABCDEF
_REF = {}


def _ref(name, c):
    """(map, ring table, vertices, cracks) of the reference, computed once and shared by the tests (read-only)"""
    if (name, c) not in _REF:
        m = MAPS[name]()
        h, w = m.shape
        # the stripes' labels in closed form (the numpy labelling of a million pixels takes minutes): the stripe's first pixel
        label = np.broadcast_to(((np.arange(w) >> 1) << 1).astype(np.int32), (h, w)) if name.startswith("stripes") else None
        table, verts = R.rings(m, c, label=label)
        _REF[name, c] = (m, table, verts, len(R.cracks(m)))
        for a in _REF[name, c][:3]:
            a.setflags(write=False)
    return _REF[name, c]


def _labels(md, h, w, c):
    from drs_amd import _lib
    label = torch.empty(h * w, dtype=torch.int32, device=DEV)
    size = torch.empty(h * w, dtype=torch.int32, device=DEV)
    _lib.call("drs_components", md.data_ptr(), h, w, c, label.data_ptr(), size.data_ptr(), stream())
    return label


def _rings(md, label, h, w, c, cap, fill):
    """one drs_polygon_rings into a scratch that holds the byte `fill`: (scratch, counters as a list)"""
    from drs_amd import _lib
    nbytes = _lib.query("drs_polygon_scratch_bytes", h, w, cap)
    assert nbytes > 0
    scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    counters = torch.full((4,), 12345, dtype=torch.int64, device=DEV)
    _lib.call("drs_polygon_rings", md.data_ptr(), label.data_ptr(), h, w, c, cap, scratch.data_ptr(), counters.data_ptr(), stream())
    torch.cuda.synchronize()
    return scratch, counters.cpu().tolist()


GUARD = 8


def _write(scratch, h, w, cap, rings, vertices, ring_cap=None, vertex_cap=None, fill=None):
    """one drs_polygon_write into outputs of exactly (rings, vertices) elements followed by GUARD guard words, everything pre-filled
    with SENTINEL (or the byte `fill`): (table, vertices, their guard words, status)"""
    from drs_amd import _lib
    if fill is None:
        table = torch.full((rings * 7 + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
        verts = torch.full((vertices * 2 + GUARD,), SENTINEL & 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    else:
        table = torch.full(((rings * 7 + GUARD) * 8,), fill, dtype=torch.uint8, device=DEV).view(torch.int64)
        verts = torch.full(((vertices * 2 + GUARD) * 4,), fill, dtype=torch.uint8, device=DEV).view(torch.int32)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    _lib.call("drs_polygon_write", scratch.data_ptr(), h, w, cap, rings if ring_cap is None else ring_cap,
              vertices if vertex_cap is None else vertex_cap, table.data_ptr(), verts.data_ptr(), status.data_ptr(), stream())
    torch.cuda.synchronize()
    table, verts = table.cpu().numpy(), verts.cpu().numpy()
    return table[:rings * 7].reshape(rings, 7), verts[:vertices * 2].reshape(vertices, 2), (table[rings * 7:], verts[vertices * 2:]), int(status.item())


def _untouched(table, verts, guards, fill=None):
    t, v = (SENTINEL, SENTINEL & 0x7FFFFFFF) if fill is None else (np.full(1, fill, np.uint8).repeat(8).view(np.int64)[0],
                                                                  np.full(1, fill, np.uint8).repeat(4).view(np.int32)[0])
    return (table == t).all() and (verts == v).all() and (guards[0] == t).all() and (guards[1] == v).all()


# ------------------------------------------------------------------------------------------------------------- 1. equality
@pytest.mark.parametrize("name, c", CASES)
def test_rings_and_vertices_equal_the_reference(name, c):
    from drs_amd import _lib
    m, want_table, want_verts, want_cracks = _ref(name, c)
    h, w = m.shape
    md = dev(np.array(m).reshape(-1))
    label = _labels(md, h, w, c)
    count = torch.full((1,), 999, dtype=torch.int64, device=DEV)
    _lib.call("drs_polygon_count", md.data_ptr(), h, w, count.data_ptr(), stream())
    assert int(count.item()) == want_cracks
    first = None
    # the scratch and the outputs holding 0x00, then 0xFF, then 0xFF again: the same bits every time
    for fill in (0x00, 0xFF, 0xFF):
        scratch, counters = _rings(md, label, h, w, c, want_cracks, fill)
        assert counters == [want_cracks, len(want_table), len(want_verts), 0], (fill, counters)
        table, verts, guards, status = _write(scratch, h, w, want_cracks, len(want_table), len(want_verts), fill=fill)
        assert status == 0
        np.testing.assert_array_equal(table, want_table, err_msg="fill=%r" % fill)
        np.testing.assert_array_equal(verts, want_verts, err_msg="fill=%r" % fill)
        assert _untouched(table[:0], verts[:0], guards, fill=fill)
        if first is None:
            first = (table.tobytes(), verts.tobytes())
        assert (table.tobytes(), verts.tobytes()) == first
    if name == "serpentine-67x131":
        assert want_table[:, 5].max() == 8976
    if name == "uniform-300x300":
        assert want_table.tolist() == [[0, 0, 2, 0, 4, 1200, 180000]] and want_verts.tolist() == [[300, 0], [300, 300], [0, 300], [0, 0]]
    if name == "checkerboard-67x131" and c == 8:
        assert (want_table[:, 6] < 0).sum() == 8385


# ------------------------------------------------------------------------------------------------------------- 2. capacities
@pytest.mark.parametrize("name, c", CASES)
def test_a_wrong_capacity_is_a_status_word(name, c):
    m, want_table, want_verts, cracks = _ref(name, c)
    h, w = m.shape
    nr, nv = len(want_table), len(want_verts)
    md = dev(np.array(m).reshape(-1))
    label = _labels(md, h, w, c)
    # crack_cap one above the count (where 4 h w allows it): the same outputs
    if cracks + 1 <= 4 * h * w:
        scratch, counters = _rings(md, label, h, w, c, cracks + 1, 0xA5)
        assert counters == [cracks, nr, nv, 0]
        table, verts, guards, status = _write(scratch, h, w, cracks + 1, nr, nv)
        assert status == 0 and _untouched(table[:0], verts[:0], guards)
        np.testing.assert_array_equal(table, want_table)
        np.testing.assert_array_equal(verts, want_verts)
    # one below: status 1, no ring, no vertex, and drs_polygon_write leaves the outputs alone
    assert cracks > 1
    scratch, counters = _rings(md, label, h, w, c, cracks - 1, 0xA5)
    assert counters == [cracks, 0, 0, 1]
    table, verts, guards, status = _write(scratch, h, w, cracks - 1, nr, nv)
    assert status == 1 and _untouched(table, verts, guards)
    # ring_cap or vertex_cap one below what the scratch holds; a crack_cap other than the scratch's
    scratch, counters = _rings(md, label, h, w, c, cracks, 0x5A)
    assert counters == [cracks, nr, nv, 0]
    for kw in (dict(ring_cap=nr - 1), dict(vertex_cap=nv - 1), dict(ring_cap=0, vertex_cap=0)):
        table, verts, guards, status = _write(scratch, h, w, cracks, nr, nv, **kw)
        assert status == 1 and _untouched(table, verts, guards), kw
    table, verts, guards, status = _write(scratch, h, w, cracks - 1, nr, nv)
    assert status == 1 and _untouched(table, verts, guards)
    # and larger capacities than needed write exactly the elements there are
    from drs_amd import _lib
    big_t = torch.full(((nr + 3) * 7,), SENTINEL, dtype=torch.int64, device=DEV)
    big_v = torch.full(((nv + 5) * 2,), 0x55555555, dtype=torch.int32, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    _lib.call("drs_polygon_write", scratch.data_ptr(), h, w, cracks, nr + 3, nv + 5, big_t.data_ptr(), big_v.data_ptr(), status.data_ptr(), stream())
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    np.testing.assert_array_equal(big_t.cpu().numpy()[:nr * 7].reshape(nr, 7), want_table)
    np.testing.assert_array_equal(big_v.cpu().numpy()[:nv * 2].reshape(nv, 2), want_verts)
    assert (big_t.cpu().numpy()[nr * 7:] == SENTINEL).all() and (big_v.cpu().numpy()[nv * 2:] == 0x55555555).all()


# ------------------------------------------------------------------------------------------------------------- 3. arguments
def test_rejected_arguments_launch_nothing():
    from drs_amd import _lib
    m = MAPS["speckled-5x7"]()
    md = dev(np.array(m).reshape(-1))
    label = _labels(md, 5, 7, 4)
    cracks = len(R.cracks(m))
    nbytes = _lib.query("drs_polygon_scratch_bytes", 5, 7, cracks)
    scratch = torch.full((nbytes,), 0x77, dtype=torch.uint8, device=DEV)
    counters = torch.full((4,), 77, dtype=torch.int64, device=DEV)
    table = torch.full((70,), 77, dtype=torch.int64, device=DEV)
    verts = torch.full((280,), 77, dtype=torch.int32, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    good = dict(map=md.data_ptr(), label=label.data_ptr(), h=5, w=7, c=4, cap=cracks, scratch=scratch.data_ptr(), counters=counters.data_ptr())
    for kw in (dict(map=None), dict(label=None), dict(scratch=None), dict(counters=None), dict(h=0), dict(w=0), dict(w=-7),
               dict(h=1 << 14, w=(1 << 14) + 1), dict(c=0), dict(c=6), dict(cap=0), dict(cap=141), dict(cap=-3)):
        a = dict(good, **kw)
        assert _lib.query("drs_polygon_rings", *[a[k] for k in good], stream()) == 1, kw
    for args in ((None, 5, 7, counters.data_ptr()), (md.data_ptr(), 5, 7, None), (md.data_ptr(), 0, 7, counters.data_ptr()),
                 (md.data_ptr(), 1 << 14, (1 << 14) + 1, counters.data_ptr())):
        assert _lib.query("drs_polygon_count", *args, stream()) == 1, args
    goodw = dict(scratch=scratch.data_ptr(), h=5, w=7, cap=cracks, ring_cap=10, vertex_cap=140, table=table.data_ptr(), verts=verts.data_ptr(),
                 status=status.data_ptr())
    for kw in (dict(scratch=None), dict(table=None), dict(verts=None), dict(status=None), dict(h=0), dict(w=0), dict(cap=0), dict(cap=141),
               dict(ring_cap=-1), dict(vertex_cap=-1)):
        a = dict(goodw, **kw)
        assert _lib.query("drs_polygon_write", *[a[k] for k in goodw], stream()) == 1, kw
    torch.cuda.synchronize()
    assert (scratch == 0x77).all() and (counters == 77).all() and (table == 77).all() and (verts == 77).all() and (status == 77).all()
    assert _lib.query("drs_polygon_scratch_bytes", 0, 7, 4) == 0 == _lib.query("drs_polygon_scratch_bytes", 5, 7, 141)


# ------------------------------------------------------------------------------------------------------------- 4. the host layer
@pytest.mark.parametrize("c", [4, 8])
def test_loops_polygons_on_another_stream(c):
    from drs_amd import loops
    name = "speckled-45x131-K6"
    m, want_table, want_verts, cracks = _ref(name, c)
    md = dev(np.array(m))
    torch.cuda.synchronize()
    table, verts, info = loops.polygons(md, 45, 131, c)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        again = loops.polygons(md.reshape(-1), 45, 131, c, stream=stream())            # the current stream's handle: the side stream
    other = loops.polygons(md, 45, 131, c, stream=side.cuda_stream)                    # ... and from outside it
    torch.cuda.synchronize()
    for t, v, i in ((table, verts, info), again, other):
        assert t.dtype == np.int64 and v.dtype == np.int32
        np.testing.assert_array_equal(t, want_table)
        np.testing.assert_array_equal(v, want_verts)
        holes = int((want_table[:, 6] < 0).sum())
        assert i == {"rings": len(want_table), "exterior": len(want_table) - holes, "holes": holes, "vertices": len(want_verts), "cracks": cracks}
    assert info["exterior"] == len(np.unique(sieve_ref.components(m, c)[0]))
    with pytest.raises(ValueError, match="6"):
        loops.polygons(md, 45, 131, 6)
    with pytest.raises(ValueError, match="uint8"):
        loops.polygons(md.to(torch.int32), 45, 131, 4)
    with pytest.raises(ValueError, match="45 x 130"):
        loops.polygons(md, 45, 130, 4)
    for h, w in ((0, 131), (45, -1), (1 << 14, (1 << 14) + 1)):
        with pytest.raises(ValueError, match="outside h, w >= 1"):                     # the range before the tensor's shape
            loops.polygons(md, h, w, 4)


# ------------------------------------------------------------------------------------------------------------- 5. end to end
CH, K6 = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
MIN_SIZE = (9, 9, 9, 9, 4, 9)


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


def _tiles():
    from drs_amd.synthetic import make_tile
    tiles, labs = zip(*[make_tile(h, w, CH, K6, seed=s, n_seeds=30) for h, w, s in ((44, 50, 21), (37, 61, 22))])
    return list(tiles), list(labs)


def _listing(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_generate_final_maps_writes_the_polygons_of_the_written_map(tmp_path, capsys):
    from drs_amd import loops
    tiles, labs = _tiles()
    d = _net()
    names = ["3", "5"]
    args = (d, tiles, names, 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen")
    for sub in ("plain", "poly", "plain2", "sieved", "sieved_poly"):
        (tmp_path / sub).mkdir()
    capsys.readouterr()
    plain = loops.generate_final_maps(*args, str(tmp_path / "plain") + "/")
    text_plain = capsys.readouterr().out
    poly = loops.generate_final_maps(*args, str(tmp_path / "poly") + "/", polygons=4)
    text_poly = capsys.readouterr().out
    plain2 = loops.generate_final_maps(*args, str(tmp_path / "plain2") + "/")
    text_plain2 = capsys.readouterr().out
    # the return values do not change; without the option the files and the printed lines are what they were
    assert isinstance(poly, list) and len(poly) == 2
    for a, b, cc in zip(plain, poly, plain2):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, cc)
    files_plain, files_poly = _listing(str(tmp_path / "plain")), _listing(str(tmp_path / "poly"))
    assert files_plain == _listing(str(tmp_path / "plain2")) and text_plain == text_plain2
    stems = ["top_mosaic_09cm_area%s_class" % n for n in names]
    assert sorted(set(files_poly) - set(files_plain)) == sorted(s + ".geojson" for s in stems)
    assert {f: v for f, v in files_poly.items() if not f.endswith(".geojson")} == files_plain
    lines = text_poly.splitlines()
    mine = [i for i, line in enumerate(lines) if "Polygons connectivity= 4 Polygons per class= [" in line]
    assert [line for i, line in enumerate(lines) if i not in mine] == text_plain.splitlines()
    assert len(mine) == 3 and mine[-1] == len(lines) - 1 and [lines[i].split(":")[0] for i in mine] == ["Final Map 3", "Final Map 5", "Final ALL MAPS"]
    # rasterising the polygons of a class gives back the written class ids
    totals = np.zeros(K6, dtype=np.int64)
    holes = vertices = 0
    for k, stem in enumerate(stems):
        h, w = labs[k].shape
        written = np.load(str(tmp_path / "poly" / (stem + ".npy"))).reshape(h, w)
        np.testing.assert_array_equal(written, poly[k].reshape(h, w))
        doc = json.load(open(str(tmp_path / "poly" / (stem + ".geojson"))))
        feats = doc["features"]
        for cls in range(K6):
            rings = [np.array(r[:-1]) for f in feats if f["properties"]["class"] == cls for r in f["geometry"]["coordinates"]]
            np.testing.assert_array_equal(R.fill(h, w, rings), written == cls)
            assert sum(f["properties"]["pixels"] for f in feats if f["properties"]["class"] == cls) == (written == cls).sum()
            totals[cls] += sum(1 for f in feats if f["properties"]["class"] == cls)
        label = sieve_ref.components(written, 4)[0]
        assert sorted(f["properties"]["component"] for f in feats) == np.unique(label).tolist()
        assert all(r[0] == r[-1] for f in feats for r in f["geometry"]["coordinates"])
        holes += sum(len(f["geometry"]["coordinates"]) - 1 for f in feats)
        vertices += sum(len(r) - 1 for f in feats for r in f["geometry"]["coordinates"])
        want_table, want_verts = R.rings(written, 4, label=label)
        assert loops._polygons_str(4, loops._polygons_info(want_table, {"cracks": 0}, K6)) == lines[mine[k]].split(": ", 1)[1]
    assert lines[mine[-1]] == "Final ALL MAPS: Polygons connectivity= 4 Polygons per class= [%s] Holes= %d Vertices= %d" % (
        " ".join(str(v) for v in totals), holes, vertices)
    assert totals.sum() > 20 and holes > 0
    # with the sieve: the sieved map is what is traced, and no polygon is below its class's minimum mapping unit
    for c in (4, 8):
        sieve = dict(min_size=MIN_SIZE, connectivity=c)
        out = str(tmp_path / "sieved_poly") + "/c%d_" % c
        sieved = loops.generate_final_maps(*args, out, sieve=sieve, polygons=c)
        capsys.readouterr()
        for k, stem in enumerate(stems):
            h, w = labs[k].shape
            want, info = sieve_ref.sieve(plain[k].reshape(h, w), K6, MIN_SIZE, c)
            assert info["merged"] > 0 and info["left_small"] == 0
            np.testing.assert_array_equal(sieved[k].reshape(h, w), want)
            feats = json.load(open(out + stem + ".geojson"))["features"]
            assert feats and all(f["properties"]["pixels"] >= MIN_SIZE[f["properties"]["class"]] for f in feats)
            for cls in range(K6):
                rings = [np.array(r[:-1]) for f in feats if f["properties"]["class"] == cls for r in f["geometry"]["coordinates"]]
                np.testing.assert_array_equal(R.fill(h, w, rings), want == cls)
