"""-m gpu: the superpixel vote (include/drs.h drs_superpixel_features / drs_superpixels / drs_region_vote;
loops.superpixels, loops.region_vote, loops.superpixel_vote, validate_test's and generate_final_maps' superpixel) against its numpy
statement tests/superpixel_ref.py.

Every comparison is exact integer equality: after the byte features the rule is integer arithmetic; there are no tolerances."""
import ctypes

import numpy as np
import pytest
import torch

import superpixel_ref as R

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

# name: (h, w, C, S, m, iters, image kind)
CASES = {
    "nothing-divides": (37, 53, 3, 5, 10, 5, "blobs"),
    "one-pixel": (1, 1, 1, 4, 1, 1, "blobs"),
    "one-row": (1, 200, 1, 8, 10, 3, "blobs"),
    "one-column": (200, 1, 1, 8, 10, 3, "blobs"),
    "one-centre": (3, 3, 5, 32, 40, 1, "blobs"),
    "across-tiles": (70, 130, 5, 8, 20, 10, "blobs"),
    "multi-tile-16-iterations": (257, 300, 4, 16, 10, 16, "blobs"),
    "constant": (45, 70, 3, 8, 10, 4, "constant"),
    "checker3-m1": (50, 67, 2, 6, 1, 4, "checker3"),
    "noise-m1": (66, 70, 8, 4, 1, 5, "noise"),
    "two-valued-noise-m1": (66, 70, 2, 4, 1, 8, "noise2"),
}
K6 = 6
_REF = {}


def _ref(name):
    """the reference of a case, computed once and shared by the tests (read-only)"""
    if name not in _REF:
        h, w, C, S, m, iters, kind = CASES[name]
        tile = R.image(h, w, C, 7, kind)
        lo, inv = R.scale_of(tile)
        feat = R.features(tile, lo, inv)
        assign, colour, centres = R.slic(feat, S, m, iters)
        label, size = R.regions(assign)
        pred = R.label_map(h, w, K6, 11)
        voted, counters = R.vote(pred, label, K6)
        _REF[name] = dict(tile=tile, lo=lo, inv=inv, feat=feat, assign=assign, colour=colour, centres=centres, label=label, size=size,
                          pred=pred, voted=voted, counters=counters)
        for v in _REF[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[name]


def _floats(v):
    return (ctypes.c_float * len(v))(*[float(x) for x in v])


def _features(tile, lo, inv, fill=0x5A):
    from drs_amd import _lib
    h, w, C = tile.shape
    feat = torch.full((h, w, C), fill, dtype=torch.uint8, device=DEV)
    td = dev(np.array(tile))
    a, b = _floats(lo), _floats(inv)
    _lib.call("drs_superpixel_features", td.data_ptr(), 1 if tile.dtype == np.float64 else 0, C, h, w, ctypes.addressof(a), ctypes.addressof(b),
              feat.data_ptr(), stream())
    torch.cuda.synchronize()
    return feat


def _slic(feat, S, m, iters, fill=None):
    """drs_superpixels on a device feature map; fill: the byte the scratch holds before.  Returns device tensors."""
    from drs_amd import _lib
    h, w, C = feat.shape
    need = _lib.query("drs_superpixel_scratch_bytes", C, h, w, S)
    gh, gw = R.grid(h, w, S)
    assert need == 4 * gh * gw * (C + 3)
    scratch = torch.full((need,), 0 if fill is None else fill, dtype=torch.uint8, device=DEV)
    assign = torch.full((h, w), -7, dtype=torch.int32, device=DEV)
    colour = torch.full((h, w), 99, dtype=torch.uint8, device=DEV)
    centres = torch.full((gh * gw, C + 3), -7, dtype=torch.int32, device=DEV)
    _lib.call("drs_superpixels", feat.data_ptr(), C, h, w, S, m, iters, assign.data_ptr(), colour.data_ptr(), centres.data_ptr(),
              scratch.data_ptr(), stream())
    torch.cuda.synchronize()
    return assign, colour, centres


def _components(colour):
    from drs_amd import _lib
    h, w = colour.shape
    label = torch.full((h, w), -7, dtype=torch.int32, device=DEV)
    size = torch.full((h, w), -7, dtype=torch.int32, device=DEV)
    _lib.call("drs_components", colour.data_ptr(), h, w, 4, label.data_ptr(), size.data_ptr(), stream())
    torch.cuda.synchronize()
    return label, size


def _vote(m, label, K, weight=None, in_place=False, fill=0xFF):
    """drs_region_vote on numpy inputs; returns (numpy map, [regions, changed])"""
    from drs_amd import _lib
    h, w = m.shape
    src = dev(np.array(m))
    ld = label if isinstance(label, torch.Tensor) else dev(np.array(label, dtype=np.int32))
    wd = None if weight is None else dev(np.array(weight))
    need = _lib.query("drs_region_vote_scratch_bytes", h, w)
    assert need == 16 * h * w
    scratch = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
    counters = torch.full((2,), 12345, dtype=torch.int32, device=DEV)
    dst = src if in_place else torch.full((h, w), 99, dtype=torch.uint8, device=DEV)
    _lib.call("drs_region_vote", src.data_ptr(), ld.data_ptr(), None if wd is None else wd.data_ptr(), h, w, K, scratch.data_ptr(),
              dst.data_ptr(), counters.data_ptr(), stream())
    torch.cuda.synchronize()
    if not in_place:
        np.testing.assert_array_equal(src.cpu().numpy(), m)                          # the input of the out-of-place form is untouched
    return dst.cpu().numpy(), counters.cpu().tolist()


# ------------------------------------------------------------------------------------------------------------- 1. the whole chain
@pytest.mark.parametrize("name", list(CASES))
def test_chain_matches_the_reference_bit_for_bit(name):
    h, w, C, S, m, iters, kind = CASES[name]
    ref = _ref(name)
    feat = _features(ref["tile"], ref["lo"], ref["inv"])
    np.testing.assert_array_equal(feat.cpu().numpy(), ref["feat"])
    assign, colour, centres = _slic(feat, S, m, iters, fill=0xFF)
    np.testing.assert_array_equal(assign.cpu().numpy(), ref["assign"])
    np.testing.assert_array_equal(colour.cpu().numpy(), ref["colour"])
    np.testing.assert_array_equal(centres.cpu().numpy(), ref["centres"])
    label, size = _components(colour)
    np.testing.assert_array_equal(label.cpu().numpy(), ref["label"])
    np.testing.assert_array_equal(size.cpu().numpy(), ref["size"])
    got, counters = _vote(ref["pred"], label, K6)
    np.testing.assert_array_equal(got, ref["voted"])
    assert counters == ref["counters"]
    # the lemma on the device's own output: 4-neighbours differ in centre exactly where they differ in colour
    a, c = assign.cpu().numpy(), colour.cpu().numpy()
    assert ((a[:, 1:] != a[:, :-1]) == (c[:, 1:] != c[:, :-1])).all() and ((a[1:] != a[:-1]) == (c[1:] != c[:-1])).all()
    # two runs give the same bits, whatever the scratch held
    again = _slic(feat, S, m, iters, fill=0x00)
    assert torch.equal(again[0], assign) and torch.equal(again[1], colour) and torch.equal(again[2], centres)
    # the comparisons cannot pass vacuously
    gh, gw = R.grid(h, w, S)
    if name == "noise-m1":
        assert (ref["size"] == 1).sum() > 2000                                       # fragments of one pixel, ten per centre
    if name == "two-valued-noise-m1":
        assert (ref["centres"][:, -1] == 0).sum() > 5 and (ref["size"] == 1).sum() > 1000           # empty centres, fragments of one pixel
    if name == "checker3-m1":
        assert len(np.unique(ref["label"])) > 2 * gh * gw and (ref["centres"][:, -1] == 0).any()     # many fragments; empty centres
    if name == "constant":
        assert len(np.unique(ref["feat"])) == 1 and len(np.unique(ref["label"])) == gh * gw
    if h * w > 9:
        assert ref["counters"][1] > 0


# ------------------------------------------------------------------------------------------------------------- 2. features
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_features_quantise_fp32_and_fp64_tiles(dtype):
    rng = np.random.default_rng(3)
    tile = (rng.standard_normal((19, 23, 5)) * 40).astype(dtype)
    tile[:, :, 3] = 2.5                                                              # a channel with max == min
    lo, inv = R.scale_of(tile)
    assert inv[3] == 0
    want = R.features(tile, lo, inv)
    np.testing.assert_array_equal(_features(tile, lo, inv).cpu().numpy(), want)
    assert want[:, :, 3].max() == 0 and want[:, :, 0].min() == 0 and want[:, :, 0].max() == 255
    # NaN and infinities, values beyond the scale on both sides, exact halves (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 254.5 -> 254)
    tile = tile.copy()
    tile[0, :7, 0] = [np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0]
    tile[1, :6, 1] = [0.5, 1.5, 2.5, 254.5, 255.0, 255.5]
    tile[2, :3, 3] = [np.nan, np.inf, 7.0]
    lo = np.array([-3.0, 0.0, 1.0, 2.5, 0.0], dtype=np.float32)
    inv = np.array([0.7, 1.0, 1.0 / 3.0, 0.0, 1e-3], dtype=np.float32)
    want = R.features(tile, lo, inv)
    assert want[1, :6, 1].tolist() == [0, 2, 2, 254, 255, 255] and want[0, :5, 0].tolist() == [0, 255, 0, 255, 0] and want[2, :3, 3].tolist() == [0, 0, 0]
    np.testing.assert_array_equal(_features(tile, lo, inv).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------- 3. the vote
@pytest.mark.parametrize("weights", ["none", "random", "zero"])
def test_vote_with_and_without_weights(weights):
    ref = _ref("across-tiles")
    h, w = ref["pred"].shape
    rng = np.random.default_rng(5)
    weight = {"none": None, "random": rng.integers(0, 256, size=(h, w), dtype=np.uint8), "zero": np.zeros((h, w), dtype=np.uint8)}[weights]
    want, want_counters = R.vote(ref["pred"], ref["label"], K6, weight)
    got, counters = _vote(ref["pred"], ref["label"], K6, weight)
    np.testing.assert_array_equal(got, want)
    assert counters == want_counters
    # map_out == map_in gives the same map, and the scratch's content does not matter
    got2, counters2 = _vote(ref["pred"], ref["label"], K6, weight, in_place=True, fill=0x00)
    np.testing.assert_array_equal(got2, want)
    assert counters2 == want_counters
    if weights == "zero":
        assert want_counters[1] == 0 and (want == ref["pred"]).all()
    else:
        assert want_counters[1] > 0
    if weights == "random":
        assert (want != ref["voted"]).any()                                          # the weights decide somewhere


def test_bytes_beyond_K_neither_vote_nor_change():
    ref = _ref("across-tiles")
    h, w = ref["pred"].shape
    m = R.label_map(h, w, 3, 21, beyond=True)
    for K in (3, 32):
        want, want_counters = R.vote(m, ref["label"], K)
        got, counters = _vote(m, ref["label"], K)
        np.testing.assert_array_equal(got, want)
        assert counters == want_counters and want_counters[1] > 0
        assert (got[m >= K] == m[m >= K]).all() and ((got >= K) == (m >= K)).all() and (m >= K).any()


def test_vote_works_on_any_labelling_with_large_regions():
    """regions far larger than a wavefront's run (the sums of a whole wavefront combine) and a map that is one region"""
    h, w = 96, 301
    m = R.label_map(h, w, 4, 31)
    rng = np.random.default_rng(8)
    weight = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    halves = np.zeros((h, w), dtype=np.int32)
    halves[:, 150:] = 150
    for label in (np.zeros((h, w), dtype=np.int32), halves):
        for wt in (None, weight):
            want, want_counters = R.vote(m, label, 4, wt)
            got, counters = _vote(m, label, 4, wt)
            np.testing.assert_array_equal(got, want)
            assert counters == want_counters


# ------------------------------------------------------------------------------------------------------------- 4. arguments
def test_rejected_arguments_launch_nothing():
    from drs_amd import _lib
    ref = _ref("nothing-divides")
    h, w, C, S, m, iters, _ = CASES["nothing-divides"]
    td = dev(np.array(ref["tile"]))
    lo, inv = _floats(ref["lo"]), _floats(ref["inv"])
    feat = torch.full((h, w, C), 77, dtype=torch.uint8, device=DEV)
    good = dict(tile=td.data_ptr(), f64=0, C=C, h=h, w=w, lo=ctypes.addressof(lo), inv=ctypes.addressof(inv), feat=feat.data_ptr())
    for kw in (dict(tile=None), dict(lo=None), dict(inv=None), dict(feat=None), dict(C=0), dict(C=9), dict(h=0), dict(w=0), dict(h=32769),
               dict(w=-3), dict(f64=2)):
        a = dict(good, **kw)
        assert _lib.query("drs_superpixel_features", *[a[k] for k in good], stream()) == 1, kw
    torch.cuda.synchronize()
    assert (feat == 77).all()

    fd = dev(np.array(ref["feat"]))
    gh, gw = R.grid(h, w, S)
    assign = torch.full((h, w), 77, dtype=torch.int32, device=DEV)
    colour = torch.full((h, w), 77, dtype=torch.uint8, device=DEV)
    centres = torch.full((gh * gw, C + 3), 77, dtype=torch.int32, device=DEV)
    scratch = torch.full((gh * gw * (C + 3),), 77, dtype=torch.int32, device=DEV)
    good = dict(feat=fd.data_ptr(), C=C, h=h, w=w, S=S, m=m, iters=iters, assign=assign.data_ptr(), colour=colour.data_ptr(),
                centres=centres.data_ptr(), scratch=scratch.data_ptr())
    for kw in (dict(feat=None), dict(assign=None), dict(colour=None), dict(centres=None), dict(scratch=None), dict(C=0), dict(C=9), dict(h=0),
               dict(w=0), dict(w=32769), dict(S=3), dict(S=33), dict(m=0), dict(m=41), dict(iters=0), dict(iters=17)):
        a = dict(good, **kw)
        assert _lib.query("drs_superpixels", *[a[k] for k in good], stream()) == 1, kw
    torch.cuda.synchronize()
    assert (assign == 77).all() and (colour == 77).all() and (centres == 77).all() and (scratch == 77).all()

    md, ld = dev(np.array(ref["pred"])), dev(np.array(ref["label"]))
    out = torch.full((h, w), 77, dtype=torch.uint8, device=DEV)
    counters = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    vs = torch.full((2 * h * w,), 77, dtype=torch.int64, device=DEV)
    good = dict(map_in=md.data_ptr(), label=ld.data_ptr(), weight=None, h=h, w=w, K=K6, scratch=vs.data_ptr(), map_out=out.data_ptr(),
                counters=counters.data_ptr())
    for kw in (dict(map_in=None), dict(label=None), dict(scratch=None), dict(map_out=None), dict(counters=None), dict(h=0), dict(w=0),
               dict(h=32769), dict(K=0), dict(K=33)):
        a = dict(good, **kw)
        assert _lib.query("drs_region_vote", *[a[k] for k in good], stream()) == 1, kw
    torch.cuda.synchronize()
    assert (out == 77).all() and (counters == 77).all() and (vs == 77).all()
    assert _lib.query("drs_superpixel_scratch_bytes", 9, h, w, S) == 0 == _lib.query("drs_region_vote_scratch_bytes", 0, w)


# ------------------------------------------------------------------------------------------------------------- 5. the loops
CH = 5
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
CRF = dict(iters=2, radius=3, step=1, w_app=4.0, theta_xy=8.0, theta_rgb=0.08, w_smooth=2.0, theta_s=2.0)
SIEVE = dict(min_size=(9, 9, 9, 9, 4, 9), connectivity=8)
SPX = dict(size=6, compactness=8, iters=3)
_SHARED = {}


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
    if "tiles" not in _SHARED:
        tiles, labs = zip(*[make_tile(h, w, CH, K6, seed=s, n_seeds=30) for h, w, s in ((44, 50, 21), (37, 61, 22))])
        _SHARED["tiles"] = (list(tiles), list(labs))
    return _SHARED["tiles"]


def _ref_regions(k):
    """the reference's region labels of synthetic tile k at SPX, computed once"""
    if ("regions", k) not in _SHARED:
        tile = _tiles()[0][k]
        lo, inv = R.scale_of(tile)
        assign, _, centres = R.slic(R.features(tile, lo, inv), SPX["size"], SPX["compactness"], SPX["iters"])
        _SHARED["regions", k] = (R.regions(assign)[0], int(centres.shape[0]))
    return _SHARED["regions", k]


def _ref_vote(k, m0, weight=None):
    label, ncentres = _ref_regions(k)
    out, (nreg, changed) = R.vote(m0.reshape(label.shape), label, K6, weight)
    return out, {"regions": nreg, "changed_pixels": changed, "centres": ncentres}


def test_loops_superpixels_and_region_vote_are_thin_calls():
    from drs_amd import loops, patches
    tiles, labs = _tiles()
    pool = patches.TilePool(tiles, labs, DEV)
    for k in (0, 1):
        h, w = labs[k].shape
        lo, inv = loops.superpixel_scale(pool, k)
        want_lo, want_inv = R.scale_of(tiles[k])
        assert lo.dtype == np.float32 == inv.dtype and lo.tobytes() == want_lo.tobytes() and inv.tobytes() == want_inv.tobytes()
        assign, label, size, centres = loops.superpixels(pool, k, SPX)
        again = loops.superpixels(pool, k, patches.check_superpixel(SPX), stream=stream())
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((assign, label, size, centres), again))
        feat = R.features(tiles[k], want_lo, want_inv)
        want_assign, _, want_centres = R.slic(feat, SPX["size"], SPX["compactness"], SPX["iters"])
        np.testing.assert_array_equal(assign.cpu().numpy(), want_assign)
        np.testing.assert_array_equal(centres.cpu().numpy(), want_centres)
        want_label, want_size = R.regions(want_assign)
        np.testing.assert_array_equal(label.cpu().numpy(), want_label)
        np.testing.assert_array_equal(size.cpu().numpy(), want_size)
        np.testing.assert_array_equal(want_label, _ref_regions(k)[0])
        m = R.label_map(h, w, K6, 40 + k)
        got, info = loops.region_vote(dev(m), label, h, w, K6)
        want, counters = R.vote(m, want_label, K6)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert info == {"regions": counters[0], "changed_pixels": counters[1]}
    with pytest.raises(ValueError, match="uint8"):
        loops.region_vote(dev(m).to(torch.int32), label, h, w, K6)
    with pytest.raises(ValueError, match="int32"):
        loops.region_vote(dev(m), label.to(torch.int64), h, w, K6)
    with pytest.raises(ValueError, match="size 2"):
        loops.superpixels(pool, 0, 2)


def _superpixel_lines(text):
    return [i for i, line in enumerate(text.splitlines()) if ": Superpixel size= " in line]


@pytest.mark.parametrize("options", [{}, dict(crf=CRF), dict(sieve=SIEVE)], ids=["alone", "crf", "sieve"])
def test_validate_test_votes_before_the_sieve_and_after_the_crf(capsys, options):
    import sieve_ref
    from drs_amd import loops
    tiles, labs = _tiles()
    d = _net()
    unvoted = {key: v for key, v in options.items() if key != "sieve"}                   # the run whose maps the vote starts from
    capsys.readouterr()
    res0 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **unvoted)
    text0 = capsys.readouterr().out
    cm1, maps1, extra = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, superpixel=SPX, **options)
    text1 = capsys.readouterr().out
    sp = extra["superpixel"]
    assert set(extra) == ({"superpixel", "sieve"} if "sieve" in options else {"superpixel"})
    for k, (m0, m1, lab) in enumerate(zip(res0[1], maps1, labs)):
        want, info = _ref_vote(k, m0)
        assert sp["per_map"][k] == info and info["changed_pixels"] > 0
        if "sieve" in options:
            want, sinfo = sieve_ref.sieve(want, K6, SIEVE["min_size"], 8)
            assert extra["sieve"]["per_map"][k] == sinfo
        np.testing.assert_array_equal(m1.reshape(lab.shape), want)
    assert sp["params"] == (6, 8, 3, "labels")
    assert sp["regions"] == sum(i["regions"] for i in sp["per_map"]) and sp["changed_pixels"] == sum(i["changed_pixels"] for i in sp["per_map"])
    # the Superpixel lines: one per map and one for all maps
    lines1 = text1.splitlines()
    mine = _superpixel_lines(text1)
    assert len(mine) == 3 and not _superpixel_lines(text0)
    for i, who, infos in zip(mine, ("Test Map a: ", "Test Map b: ", "Test ALL MAPS: "), (sp["per_map"][0], sp["per_map"][1], sp["per_map"])):
        assert lines1[i] == "---- Iter 7 -- " + who + loops._superpixel_str(sp["params"], infos)
    assert lines1[mine[-1]].endswith("Superpixel size= 6 compactness= 8 iters= 3 weight= labels Regions= %d Changed Pixels= %d"
                                     % (sp["regions"], sp["changed_pixels"]))
    if "sieve" in options:
        sieve_lines = [i for i, line in enumerate(lines1) if ": Sieve min= " in line]
        assert [i + 1 for i in mine] == sieve_lines                                      # each right before its Sieve line
    # without the option: the same call as ever, the same maps and the same output
    res2 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **unvoted)
    assert capsys.readouterr().out == text0 and len(res2) == len(res0) == 2
    np.testing.assert_array_equal(res2[0], res0[0])
    for m0, m2 in zip(res0[1], res2[1]):
        np.testing.assert_array_equal(m0, m2)


@pytest.mark.parametrize("score_maps", [None, ("margin",)], ids=["no-score-maps", "score-maps"])
def test_validate_test_votes_by_confidence_with_and_without_score_maps(capsys, score_maps):
    from drs_amd import loops
    tiles, labs = _tiles()
    d = _net()
    # the unvoted run, with score maps either way: its confidence maps are the weights
    _, maps0, extra0 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, score_maps=("margin",))
    text0 = capsys.readouterr().out
    spec = dict(SPX, weight="confidence")
    res = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, superpixel=spec, score_maps=score_maps)
    text1 = capsys.readouterr().out
    maps1, extra = res[1], res[2]
    differs = False
    for k, (m0, m1, lab) in enumerate(zip(maps0, maps1, labs)):
        conf = extra0["scores"][k]["confidence"].reshape(lab.shape)
        want, info = _ref_vote(k, m0, conf)
        np.testing.assert_array_equal(m1.reshape(lab.shape), want)
        assert extra["superpixel"]["per_map"][k] == info and info["changed_pixels"] > 0
        differs = differs or (want != _ref_vote(k, m0)[0]).any()
    assert differs                                                                       # the confidence decides somewhere
    assert extra["superpixel"]["params"].weight == "confidence" and len(_superpixel_lines(text1)) == 3
    cal = lambda text: [s for s in text.splitlines() if "Calibration ECE=" in s]
    if score_maps is None:
        assert set(extra) == {"superpixel"} and not cal(text1)                           # asked of the path, not reported
    else:
        # score maps and calibration stay those of the unvoted labels
        assert {"superpixel", "scores", "reliability", "calibration"} == set(extra)
        np.testing.assert_array_equal(extra["reliability"], extra0["reliability"])
        for k in (0, 1):
            assert set(extra["scores"][k]) == set(extra0["scores"][k]) == {"margin", "confidence"}
            for kind in extra0["scores"][k]:
                np.testing.assert_array_equal(extra["scores"][k][kind], extra0["scores"][k][kind])
        assert cal(text0) == cal(text1) and len(cal(text0)) == 3


def test_generate_final_maps_returns_what_validate_test_returns(tmp_path, capsys):
    from drs_amd import loops
    tiles, labs = _tiles()
    d = _net()
    for spec in (SPX, dict(SPX, weight="confidence")):
        _, want, _ = loops.validate_test(d, tiles, labs, ["3", "5"], 6, MEAN, STD, 25, 7, superpixel=spec, sieve=SIEVE)
        got = loops.generate_final_maps(d, tiles, ["3", "5"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen",
                                        str(tmp_path) + "/v_", superpixel=spec, sieve=SIEVE)
        plain = loops.generate_final_maps(d, tiles, ["3", "5"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", str(tmp_path) + "/p_")
        capsys.readouterr()
        assert isinstance(got, list) and len(got) == 2
        for k in (0, 1):
            np.testing.assert_array_equal(got[k], want[k])
            assert (got[k] != plain[k]).any()
        np.testing.assert_array_equal(np.load(str(tmp_path) + "/v_top_mosaic_09cm_area3_class.npy"), want[0])
    # score maps that do not name the confidence: it is asked of the path for the vote and neither returned nor written
    maps, scores = loops.generate_final_maps(d, tiles, ["3", "5"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen",
                                             str(tmp_path) + "/s_", superpixel=spec, sieve=SIEVE, score_maps=("margin",))
    capsys.readouterr()
    for k in (0, 1):
        np.testing.assert_array_equal(maps[k], want[k])
        assert set(scores[k]) == {"margin"}
    assert (tmp_path / "s_top_mosaic_09cm_area3_class_margin.npy").is_file()
    assert not (tmp_path / "s_top_mosaic_09cm_area3_class_confidence.npy").exists()
