"""-m gpu: connected components, the sieve round, the sieve and the object census (include/drs.h drs_components /
drs_sieve_round / drs_component_census; loops.components, loops.sieve_labels, validate_test's and generate_final_maps' sieve) against
their numpy statement tests/sieve_ref.py.

Every comparison is exact integer equality: the rule is integer arithmetic, there are no tolerances and no excluded pixels."""
import ctypes

import numpy as np
import pytest
import torch

import sieve_ref

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

# the tile of the labelling kernels is 32 x 32: ragged against it in both axes with several tiles; K 8; one-pixel-wide maps; a map
# smaller than a tile; one whole tile pair of one component; a component above 65 535 pixels; every pixel its own component (4) or two
# components (8); one corridor crossing every tile border many times
MAPS = {
    "speckled-45x131-K6": lambda: sieve_ref.speckled(45, 131, 6),
    "speckled-33x65-K8": lambda: sieve_ref.speckled(33, 65, 8),
    "speckled-1x40": lambda: sieve_ref.speckled(1, 40, 3),
    "speckled-40x1": lambda: sieve_ref.speckled(40, 1, 3),
    "speckled-5x7": lambda: sieve_ref.speckled(5, 7, 2),
    "uniform-64x64": lambda: sieve_ref.uniform(64, 64),
    "uniform-300x300": lambda: sieve_ref.uniform(300, 300),
    "checkerboard-67x131": lambda: sieve_ref.checkerboard(67, 131),
    "serpentine-67x131": lambda: sieve_ref.serpentine(67, 131),
    "rings": lambda: sieve_ref.rings(),
    "noise-64x64-K4": lambda: sieve_ref.noise(),
}
# (map, K, min_size): a scalar threshold; per-class thresholds with a 0; the ring map; the noise map; nothing but small components
SIEVES = [("speckled-45x131-K6", 6, 12), ("speckled-33x65-K8", 8, (5, 0, 9, 3, 20, 7, 7, 2)), ("speckled-1x40", 3, 4), ("speckled-40x1", 3, 4),
          ("rings", 3, 200), ("noise-64x64-K4", 4, 16), ("speckled-5x7", 2, 100)]
SIEVE_IDS = [s[0] + "-min" + ("".join(str(v) for v in s[2]) if isinstance(s[2], tuple) else str(s[2])) for s in SIEVES]
_MAPS, _COMPONENTS, _SIEVED = {}, {}, {}


def _map(name):
    if name not in _MAPS:
        _MAPS[name] = MAPS[name]()
        _MAPS[name].setflags(write=False)
    return _MAPS[name]


def _ref_components(name, c):
    """the reference labels and sizes of a map, computed once and shared by the tests (read-only)"""
    if (name, c) not in _COMPONENTS:
        label, size = sieve_ref.components(_map(name), c)
        label.setflags(write=False)
        size.setflags(write=False)
        _COMPONENTS[name, c] = (label, size)
    return _COMPONENTS[name, c]


def _ref_sieve(name, K, min_size, c):
    if (name, K, min_size, c) not in _SIEVED:
        out, info = sieve_ref.sieve(_map(name), K, min_size, c)
        out.setflags(write=False)
        _SIEVED[name, K, min_size, c] = (out, info)
    return _SIEVED[name, K, min_size, c]


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _components(m, c):
    from drs_amd import _lib
    h, w = m.shape
    md = dev(np.array(m).reshape(-1))
    label = torch.full((h * w,), -7, dtype=torch.int32, device=DEV)
    size = torch.full((h * w,), -7, dtype=torch.int32, device=DEV)
    _lib.call("drs_components", md.data_ptr(), h, w, c, label.data_ptr(), size.data_ptr(), stream())
    torch.cuda.synchronize()
    return md, label, size


def _np(label, size, h, w):
    return label.cpu().numpy().reshape(h, w), size.cpu().numpy().view(np.uint32).reshape(h, w)


def _thresholds(K, min_size):
    return tuple(min_size) if isinstance(min_size, tuple) else (min_size,) * K


def _round(md, label, size, h, w, K, min_size, out=None, fill=None):
    """one drs_sieve_round; out None = in place on a copy of the map; fill: the byte the scratch holds before"""
    from drs_amd import _lib
    ms = _ints(_thresholds(K, min_size))
    nbytes = _lib.query("drs_sieve_scratch_bytes", h, w)
    assert nbytes == 8 * h * w
    scratch = torch.full((nbytes,), 0 if fill is None else fill, dtype=torch.uint8, device=DEV)
    counters = torch.full((2,), 12345, dtype=torch.int32, device=DEV)
    src = md.clone()
    dst = src if out is None else out
    _lib.call("drs_sieve_round", src.data_ptr(), label.data_ptr(), size.data_ptr(), h, w, K, ctypes.addressof(ms), scratch.data_ptr(),
              dst.data_ptr(), counters.data_ptr(), stream())
    torch.cuda.synchronize()
    return dst.cpu().numpy().reshape(h, w), counters.cpu().tolist()


# ------------------------------------------------------------------------------------------------------------- 1. components
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name", [n for n in MAPS if n not in ("rings", "noise-64x64-K4")])
def test_components(name, c):
    m = _map(name)
    h, w = m.shape
    want_label, want_size = _ref_components(name, c)
    _, label, size = _components(m, c)
    got_label, got_size = _np(label, size, h, w)
    np.testing.assert_array_equal(got_label, want_label)
    np.testing.assert_array_equal(got_size, want_size)
    if name == "uniform-300x300":
        assert (got_label == 0).all() and (got_size == 90000).all()                  # no 16-bit size anywhere
    if name == "checkerboard-67x131":
        assert len(np.unique(got_label)) == (67 * 131 if c == 4 else 2)
    if name == "serpentine-67x131":
        corridor = m == 1
        assert (got_label[corridor] == 0).all() and (got_size[corridor] == corridor.sum()).all() and corridor.sum() > 4000


def test_loops_components_is_a_thin_call_and_two_runs_give_the_same_bits():
    from drs_amd import loops
    m = _map("speckled-45x131-K6")
    md = dev(np.array(m))
    for c in (4, 8):
        label, size = loops.components(md, 45, 131, c)
        again = loops.components(md.reshape(-1), 45, 131, c, stream=stream())
        torch.cuda.synchronize()
        assert label.dtype == torch.int32 and size.dtype == torch.int32 and tuple(label.shape) == (45, 131) == tuple(size.shape)
        assert torch.equal(label, again[0]) and torch.equal(size, again[1])
        np.testing.assert_array_equal(label.cpu().numpy(), _ref_components("speckled-45x131-K6", c)[0])
        np.testing.assert_array_equal(size.cpu().numpy(), _ref_components("speckled-45x131-K6", c)[1].astype(np.int32))
    with pytest.raises(ValueError, match="6"):
        loops.components(md, 45, 131, 6)
    with pytest.raises(ValueError, match="uint8"):
        loops.components(md.to(torch.int32), 45, 131, 4)


# ------------------------------------------------------------------------------------------------------------- 2. one round
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name, K, min_size", SIEVES, ids=SIEVE_IDS)
def test_one_round(name, K, min_size, c):
    m = _map(name)
    h, w = m.shape
    want, want_counters = sieve_ref.sieve_round(m, K, _thresholds(K, min_size), c)
    md, label, size = _components(m, c)
    # in place, with the scratch holding 0xFF and then 0x00; then into another buffer that holds rubbish
    for out, fill in ((None, 0xFF), (None, 0x00), (torch.full((h * w,), 99, dtype=torch.uint8, device=DEV), 0xA5)):
        got, counters = _round(md, label, size, h, w, K, min_size, out=out, fill=fill)
        np.testing.assert_array_equal(got, want, err_msg="fill=%r in_place=%r" % (fill, out is None))
        assert counters == want_counters, (fill, counters, want_counters)
    np.testing.assert_array_equal(md.cpu().numpy().reshape(h, w), m)                 # the input of the out-of-place form is untouched
    if name != "speckled-5x7":
        assert want_counters[1] > 0 and (want != m).any()                            # the comparison cannot pass vacuously


def test_a_byte_beyond_K_neither_changes_nor_spreads():
    m = np.array(_map("speckled-45x131-K6"))
    m[10:12, 20:90] = 200                                                            # a thin bar: no class pixel may take its byte
    m[30, 5] = 6
    want, want_counters = sieve_ref.sieve_round(m, 6, (12,) * 6, 4)
    md, label, size = _components(m, 4)
    got, counters = _round(md, label, size, 45, 131, 6, 12, fill=0xFF)
    np.testing.assert_array_equal(got, want)
    assert counters == want_counters
    assert (got[m >= 6] == m[m >= 6]).all() and ((got >= 6) == (m >= 6)).all()


# ------------------------------------------------------------------------------------------------------------- 3. the sieve
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name, K, min_size", SIEVES, ids=SIEVE_IDS)
def test_sieve_labels(name, K, min_size, c):
    from drs_amd import loops
    m = _map(name)
    h, w = m.shape
    want, want_info = _ref_sieve(name, K, min_size, c)
    md = dev(np.array(m))
    got, info = loops.sieve_labels(md, h, w, K, dict(min_size=list(min_size) if isinstance(min_size, tuple) else min_size, connectivity=c))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w) and got.data_ptr() != md.data_ptr()
    np.testing.assert_array_equal(md.cpu().numpy(), m)                               # the input is left alone
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert info == want_info
    assert not info["capped"] and info["rounds"] < 64
    if name == "rings":
        assert info["rounds"] == 7 and info["objects_after"] == [1, 0, 0]
    if name == "speckled-5x7":
        assert info["left_small"] > 0 and info["changed_pixels"] == 0 and info["rounds"] == 1
    else:
        assert info["left_small"] == 0 and info["rounds"] >= 2
        # a component count on the output finds nothing small
        _, label, size = _components(got.cpu().numpy(), c)
        _, size_np = _np(label, size, h, w)
        assert not sieve_ref.small_mask(got.cpu().numpy(), size_np, K, _thresholds(K, min_size)).any()
    # two runs give the same bits, on another stream handle too
    again, info2 = loops.sieve_labels(md.reshape(-1), h, w, K, dict(min_size=_thresholds(K, min_size), connectivity=c), stream=stream())
    assert torch.equal(again.reshape(h, w), got) and info2 == info


def test_the_cap_is_reported_with_what_is_left(monkeypatch):
    from drs_amd import loops, patches
    monkeypatch.setattr(patches, "SIEVE_MAX_ROUNDS", 3)                              # the ring map needs 7
    m = _map("rings")
    h, w = m.shape
    want, want_info = sieve_ref.sieve(m, 3, 200, 4, max_rounds=3)
    got, info = loops.sieve_labels(dev(np.array(m)), h, w, 3, 200)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert info == want_info and info["capped"] and info["rounds"] == 3 and info["left_small"] == 3


def test_sieve_labels_refuses_what_it_cannot_run():
    from drs_amd import loops
    md = dev(np.array(_map("speckled-5x7")))
    with pytest.raises(ValueError, match="3 given"):
        loops.sieve_labels(md, 5, 7, 2, (1, 2, 3))
    with pytest.raises(ValueError, match="-1"):
        loops.sieve_labels(md, 5, 7, 2, -1)
    with pytest.raises(ValueError, match="uint8"):
        loops.sieve_labels(md.to(torch.int32), 5, 7, 2, 3)


# ------------------------------------------------------------------------------------------------------------- 4. the census
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name, K", [("speckled-45x131-K6", 6), ("speckled-33x65-K8", 8), ("uniform-300x300", 3), ("checkerboard-67x131", 1),
                                     ("serpentine-67x131", 32)])
def test_census(name, K, c):
    from drs_amd import _lib
    m = _map(name)
    h, w = m.shape
    want_label, want_size = _ref_components(name, c)
    want = sieve_ref.census(m, want_label, want_size, K)
    md, label, size = _components(m, c)
    rng = np.random.default_rng(1)
    before = rng.integers(1, 1 << 40, size=(K, 32), dtype=np.int64)                  # the table is ADDED to
    table = dev(before.reshape(-1))
    for _ in range(2):
        _lib.call("drs_component_census", md.data_ptr(), label.data_ptr(), size.data_ptr(), h, w, K, table.data_ptr(), stream())
    torch.cuda.synchronize()
    got = (table.cpu().numpy().reshape(K, 32) - before) // 2
    np.testing.assert_array_equal(table.cpu().numpy().reshape(K, 32), before + 2 * want)
    # row sums weighted by the sizes: the pixel counts per class
    _, size_np = _np(label, size, h, w)
    roots = _np(label, size, h, w)[0].reshape(-1) == np.arange(h * w)
    for k in range(K):
        mine = roots & (m.reshape(-1) == k)
        assert got[k].sum() == mine.sum()
        assert size_np.reshape(-1)[mine].astype(np.int64).sum() == (m == k).sum()
        for b in range(32):
            assert got[k, b] == (mine & (size_np.reshape(-1) >> b == 1)).sum()


# ------------------------------------------------------------------------------------------------------------- 5. arguments
def test_rejected_arguments_launch_nothing():
    from drs_amd import _lib
    m = _map("speckled-5x7")
    md, label, size = _components(m, 4)
    out = torch.full((35,), 77, dtype=torch.uint8, device=DEV)
    counters = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(35, dtype=torch.int64, device=DEV)
    ok, neg, big = _ints((3, 3)), _ints((3, -1)), _ints((3, (1 << 30) + 1))
    good = dict(map_in=md.data_ptr(), label=label.data_ptr(), size=size.data_ptr(), h=5, w=7, K=2, min_size=ctypes.addressof(ok),
                scratch=scratch.data_ptr(), map_out=out.data_ptr(), counters=counters.data_ptr())
    bad = [dict(map_in=None), dict(label=None), dict(size=None), dict(min_size=None), dict(scratch=None), dict(map_out=None),
           dict(counters=None), dict(h=0), dict(w=0), dict(w=-7), dict(h=1 << 16, w=(1 << 14) + 1), dict(K=0), dict(K=33),
           dict(min_size=ctypes.addressof(neg)), dict(min_size=ctypes.addressof(big))]
    for kw in bad:
        a = dict(good, **kw)
        assert _lib.query("drs_sieve_round", *[a[k] for k in good], stream()) == 1, kw
    torch.cuda.synchronize()
    assert (out == 77).all() and (counters == 77).all()
    assert _lib.query("drs_sieve_scratch_bytes", 0, 7) == 0 == _lib.query("drs_sieve_scratch_bytes", 1 << 16, (1 << 14) + 1)
    assert _lib.query("drs_sieve_scratch_bytes", 1 << 15, 1 << 15) == 8 << 30


# ------------------------------------------------------------------------------------------------------------- 6. the loops
CH, K6 = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
DIST = (1, 2, 4)
CRF = dict(iters=2, radius=3, step=1, w_app=4.0, theta_xy=8.0, theta_rgb=0.08, w_smooth=2.0, theta_s=2.0)
SIEVE = dict(min_size=(9, 9, 9, 9, 4, 9), connectivity=8)


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


@pytest.mark.parametrize("options", [{}, dict(crf=CRF), dict(boundary_scores=DIST), dict(crf=CRF, boundary_scores=DIST)],
                         ids=["plain", "crf", "boundary", "crf+boundary"])
def test_validate_test_scores_the_sieved_maps(capsys, options):
    import boundary_ref
    from drs_amd import loops
    tiles, labs = _tiles()
    d = _net()
    capsys.readouterr()
    res0 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **options)
    text0 = capsys.readouterr().out
    maps0 = res0[1]
    cm1, maps1, extra = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, sieve=SIEVE, **options)
    text1 = capsys.readouterr().out
    sv = extra["sieve"]
    assert set(extra) == ({"sieve", "boundary"} if "boundary_scores" in options else {"sieve"})
    want_cm = np.zeros((K6, K6), dtype=np.int64)
    for k, (m0, m1, lab) in enumerate(zip(maps0, maps1, labs)):
        want, info = sieve_ref.sieve(m0.reshape(lab.shape), K6, SIEVE["min_size"], 8)
        np.testing.assert_array_equal(m1.reshape(lab.shape), want)
        assert sv["per_map"][k] == info and info["merged"] > 0 and info["left_small"] == 0
        want_cm += boundary_ref.confusion(lab, want, K6, 6)
        if "boundary_scores" in options:
            np.testing.assert_array_equal(extra["boundary"]["per_map"][k]["confusion"], boundary_ref.confusion(lab, want, K6, 6))
    np.testing.assert_array_equal(cm1, want_cm)
    assert (cm1 != res0[0]).any()
    if "boundary_scores" in options:
        np.testing.assert_array_equal(extra["boundary"]["hist"], sum(boundary_ref.histogram(lab, m.reshape(lab.shape), K6, 6, DIST)
                                                                     for lab, m in zip(labs, maps1)))
    assert sv["params"].min_size == SIEVE["min_size"] and sv["params"].connectivity == 8
    assert sv["merged"] == sum(i["merged"] for i in sv["per_map"]) and sv["rounds"] == max(i["rounds"] for i in sv["per_map"])
    assert sv["objects_after"] == [sum(i["objects_after"][c] for i in sv["per_map"]) for c in range(K6)]
    # the Sieve lines: one per map, after the map's other lines, and one for all maps at the end
    lines0, lines1 = text0.splitlines(), text1.splitlines()
    mine = [i for i, line in enumerate(lines1) if ": Sieve min= 9 9 9 9 4 9 connectivity= 8 Rounds= " in line]
    assert len(mine) == 3 and len(lines1) == len(lines0) + 3 and mine[-1] == len(lines1) - 1
    for i, who, infos in zip(mine, ("Test Map a: ", "Test Map b: ", "Test ALL MAPS: "), (sv["per_map"][0], sv["per_map"][1], sv["per_map"])):
        assert lines1[i] == "---- Iter 7 -- " + who + loops._sieve_str(sv["params"], infos)
    assert lines1[mine[-1]].endswith(" Merged Components= %d Changed Pixels= %d Objects per class= [%s] -> [%s]" % (
        sv["merged"], sv["changed_pixels"], " ".join(map(str, sv["objects_before"])), " ".join(map(str, sv["objects_after"]))))
    # without the option: the same call as ever, the same maps and the same output, and no third value unless another option asks
    res2 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **options)
    assert capsys.readouterr().out == text0 and len(res2) == len(res0) == (3 if "boundary_scores" in options else 2)
    np.testing.assert_array_equal(res2[0], res0[0])
    for m0, m2 in zip(maps0, res2[1]):
        np.testing.assert_array_equal(m0, m2)


def test_score_maps_stay_those_of_the_unsieved_labels(capsys):
    from drs_amd import loops
    tiles, labs = _tiles()
    d = _net()
    _, maps0, extra0 = loops.validate_test(d, tiles[:1], labs[:1], ["a"], 6, MEAN, STD, 25, 7, score_maps=("margin",))
    text0 = capsys.readouterr().out
    _, maps1, extra1 = loops.validate_test(d, tiles[:1], labs[:1], ["a"], 6, MEAN, STD, 25, 7, score_maps=("margin",), sieve=SIEVE)
    text1 = capsys.readouterr().out
    assert (maps1[0] != maps0[0]).any() and {"sieve", "scores", "reliability", "calibration"} <= set(extra1)
    np.testing.assert_array_equal(extra1["reliability"], extra0["reliability"])
    for kind in extra0["scores"][0]:
        np.testing.assert_array_equal(extra1["scores"][0][kind], extra0["scores"][0][kind])
    cal = lambda text: [s for s in text.splitlines() if "Calibration ECE=" in s]
    assert cal(text0) == cal(text1) and len(cal(text0)) == 2


def test_generate_final_maps_writes_the_sieved_maps(tmp_path, capsys):
    from drs_amd import loops
    tiles, labs = _tiles()
    d = _net()
    args = (d, tiles[:1], ["3"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen")
    plain = loops.generate_final_maps(*args, str(tmp_path) + "/plain_")
    sieved = loops.generate_final_maps(*args, str(tmp_path) + "/sieved_", sieve=SIEVE)
    capsys.readouterr()
    h, w = labs[0].shape
    want, info = sieve_ref.sieve(plain[0].reshape(h, w), K6, SIEVE["min_size"], 8)
    assert info["merged"] > 0
    np.testing.assert_array_equal(sieved[0].reshape(h, w), want)
    np.testing.assert_array_equal(np.load(str(tmp_path) + "/sieved_top_mosaic_09cm_area3_class.npy").reshape(h, w), want)
    np.testing.assert_array_equal(np.load(str(tmp_path) + "/plain_top_mosaic_09cm_area3_class.npy"), plain[0])
    assert (tmp_path / "sieved_top_mosaic_09cm_area3_class.tif").is_file()
