"""The superpixel vote without a device: the numpy statement tests/superpixel_ref.py against its own lemmas, the
option's values (patches.check_superpixel / parse_superpixel), the command line, and the argument checks of the four entry points
(include/drs.h drs_superpixel_features / drs_superpixels / drs_region_vote and the two size queries)."""
import ctypes as C

import numpy as np
import pytest
import torch

import superpixel_ref as R
from drs_amd import patches as P

# (h, w, C, S, m, iters, kind): small random cases of the reference
CASES = [(37, 53, 3, 5, 10, 5, "blobs"), (1, 1, 1, 4, 1, 1, "blobs"), (1, 60, 1, 8, 10, 3, "noise"), (60, 1, 1, 8, 10, 3, "noise"),
         (3, 3, 5, 32, 40, 1, "blobs"), (40, 45, 2, 4, 1, 4, "noise"), (33, 40, 4, 8, 1, 3, "checker3"), (30, 41, 3, 6, 7, 3, "constant")]
_SLIC = {}


def _slic(case):
    if case not in _SLIC:
        h, w, Cn, S, m, iters, kind = case
        tile = R.image(h, w, Cn, 3, kind)
        feat = R.features(tile, *R.scale_of(tile))
        _SLIC[case] = (feat,) + R.slic(feat, S, m, iters)
        for a in _SLIC[case]:
            a.setflags(write=False)
    return _SLIC[case]


# ------------------------------------------------------------------------------------------------------------- the reference's lemmas
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_ref_neighbours_with_different_centres_have_different_colours(case):
    """the lemma: the 4-connected components of the colouring are the connected pieces of the clusters"""
    _, assign, colour, _ = _slic(case)
    for a, b, ca, cb in ((assign[:, 1:], assign[:, :-1], colour[:, 1:], colour[:, :-1]),
                         (assign[1:], assign[:-1], colour[1:], colour[:-1])):
        assert ((a != b) == (ca != cb)).all()
    assert colour.max() < 16
    np.testing.assert_array_equal(R.regions(assign)[0], R.regions(colour)[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_ref_every_cluster_lies_within_its_3x3_cells(case):
    h, w, Cn, S, m, iters, _ = case
    feat, assign, _, centres = _slic(case)
    gh, gw = R.grid(h, w, S)
    assert centres.shape == (gh * gw, Cn + 3)
    ci, cj = R.cells(w, gw), R.cells(h, gh)
    assert (np.abs(assign % gw - ci[None, :]) <= 1).all() and (np.abs(assign // gw - cj[:, None]) <= 1).all()
    # the counts are those of the last assignment, and the centres stay inside the 3 x 3 cells too
    np.testing.assert_array_equal(centres[:, -1], np.bincount(assign.reshape(-1), minlength=gh * gw))
    ids = np.arange(gh * gw)
    assert (np.abs(ci[centres[:, 0]] - ids % gw) <= 1).all() and (np.abs(cj[centres[:, 1]] - ids // gw) <= 1).all()
    assert centres[:, 2:-1].min() >= 0 and centres[:, 2:-1].max() <= 255


def test_ref_features_quantise_in_fp32_steps():
    lo, inv = np.array([0.5, 1.0], dtype=np.float32), np.array([64.0, 0.0], dtype=np.float32)
    s = 1.0 / 128                                              # t = 0, 0.5, 1.5, NaN, 544, < 0, 2.5 in channel 0: all exact in fp32
    tile = np.array([[[0.5, 7.0], [0.5 + s, np.inf], [0.5 + 3 * s, -np.inf], [np.nan, np.nan], [9.0, 1.0], [0.4, 2.0], [0.5 + 5 * s, 0.0]]],
                    dtype=np.float64)
    want = [[0, 0], [0, 0], [2, 0], [0, 0], [255, 0], [0, 0], [2, 0]]          # 0.5 -> 0 and 2.5 -> 2: half to even; inf * 0 = NaN -> 0
    got = R.features(tile, lo, inv)
    assert got.dtype == np.uint8 and got.tolist() == [want]
    t = R.image(9, 11, 3, 1)
    t[:, :, 1] = 4.0
    lo, inv = R.scale_of(t)
    assert inv[1] == 0 and lo[1] == 4 and inv.dtype == np.float32 == lo.dtype
    f = R.features(t, lo, inv)
    assert f[:, :, 1].max() == 0 and f[:, :, 0].min() == 0 and f[:, :, 0].max() == 255


def test_ref_regions_are_flood_fills():
    ids = np.array([[1, 1, 2], [3, 1, 2], [3, 3, 1]])
    label, size = R.regions(ids)
    assert label.tolist() == [[0, 0, 2], [3, 0, 2], [3, 3, 8]] and size.tolist() == [[3, 3, 2], [3, 3, 2], [3, 3, 1]]


# ------------------------------------------------------------------------------------------------------------- the vote
def test_ref_after_a_vote_every_region_holds_one_class_among_its_bytes_below_K():
    for seed, K, beyond in ((1, 6, False), (2, 3, True), (3, 32, True)):
        m = R.label_map(31, 47, K, seed, beyond)
        label, _ = R.regions(R.label_map(31, 47, 9, seed + 10))
        rng = np.random.default_rng(seed)
        for weight in (None, rng.integers(0, 256, size=m.shape, dtype=np.uint8)):
            out, (nreg, changed) = R.vote(m, label, K, weight)
            assert nreg == len(np.unique(label)) and changed == (out != m).sum() and changed > 0
            np.testing.assert_array_equal(out[m >= K], m[m >= K])
            assert ((out >= K) == (m >= K)).all()
            for r in np.unique(label):
                assert len(np.unique(out[(label == r) & (out < K)])) <= 1


def test_ref_a_region_whose_largest_sum_is_zero_is_unchanged():
    m = np.array([[0, 1, 1, 2, 2, 2]], dtype=np.uint8)
    label = np.array([[0, 0, 0, 3, 3, 3]], dtype=np.int32)
    weight = np.array([[0, 0, 0, 1, 0, 0]], dtype=np.uint8)
    out, counters = R.vote(m, label, 3, weight)
    assert out.tolist() == [[0, 1, 1, 2, 2, 2]] and counters == [2, 0]
    out, counters = R.vote(m, label, 3, np.zeros_like(weight))
    assert out.tolist() == m.tolist() and counters == [2, 0]
    out, counters = R.vote(m, label, 3)
    assert out.tolist() == [[1, 1, 1, 2, 2, 2]] and counters == [2, 1]


def test_ref_ties_go_to_the_lower_class_and_weights_beat_counts():
    m = np.array([[2, 1, 1, 2, 7, 0]], dtype=np.uint8)
    label = np.zeros((1, 6), dtype=np.int32)
    out, counters = R.vote(m, label, 3)
    assert out.tolist() == [[1, 1, 1, 1, 7, 1]] and counters == [1, 3]                   # 2 : 2 between classes 1 and 2; 7 stays
    out, _ = R.vote(m, label, 3, np.array([[1, 1, 1, 1, 200, 9]], dtype=np.uint8))
    assert out.tolist() == [[0, 0, 0, 0, 7, 0]]                                          # one pixel of weight 9 beats two of 1 + 1
    out, _ = R.vote(m, label, 8, np.array([[1, 1, 1, 1, 200, 9]], dtype=np.uint8))
    assert out.tolist() == [[7] * 6]                                                     # with K = 8 the byte 7 votes too


# ------------------------------------------------------------------------------------------------------------- the option's values
def test_check_superpixel_and_parse():
    D = P.SuperpixelParams(8, 10, 5, "labels")
    assert P.SUPERPIXEL_DEFAULTS == D == P.check_superpixel(None) == P.check_superpixel(True) == P.check_superpixel({}) == P.check_superpixel(8)
    assert P.check_superpixel(16) == (16, 10, 5, "labels") == P.check_superpixel(np.int64(16)) == P.check_superpixel([16])
    assert P.check_superpixel((4, 1, 1)) == (4, 1, 1, "labels") and P.check_superpixel([32, 40, 16]) == (32, 40, 16, "labels")
    assert P.check_superpixel(dict(weight="confidence")) == (8, 10, 5, "confidence")
    assert P.check_superpixel(dict(size=12, iters=2)) == (12, 10, 2, "labels")
    got = P.check_superpixel(P.SuperpixelParams(np.int32(6), np.int64(3), 2, "confidence"))
    assert got == (6, 3, 2, "confidence") and all(type(v) is int for v in got[:3])
    assert P.parse_superpixel("8") == (8,) and P.parse_superpixel("16,20") == (16, 20) and P.parse_superpixel("4,1,16") == (4, 1, 16)


@pytest.mark.parametrize("bad, names", [
    (3, "size 3"), (33, "size 33"), (-8, "-8"), (8.0, "8.0"), (False, "False"), ("8", "'8'"), ((), "()"), ((8, 10, 5, 1), "(8, 10, 5, 1)"),
    ((8, 0), "compactness 0"), ((8, 41), "compactness 41"), ((8, 10, 0), "iters 0"), ((8, 10, 17), "iters 17"), ((8, 2.0), "2.0"),
    (dict(size=True), "True"), (dict(weight="posterior"), "'posterior'"), (dict(weight=None), "None"), (dict(step=8), "'step'"),
    (dict(size="8"), "'8'"),
])
def test_check_superpixel_names_the_offender(bad, names):
    with pytest.raises(ValueError) as e:
        P.check_superpixel(bad)
    assert names in str(e.value), str(e.value)


@pytest.mark.parametrize("bad", ["", "1.5", "8, 10", " 8", "8,", ",8", "a", "8,-2", "+8", "-8", "3", "33", "8,41", "8,10,17", "8,10,5,1", None, 8])
def test_parse_superpixel_refuses(bad):
    with pytest.raises(ValueError):
        P.parse_superpixel(bad)


# ------------------------------------------------------------------------------------------------------------- the command line
ARGV = ["x.py", "a", "b"]
MAIN_ARGV = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
             "single_fixed", "25", "acc"]


def test_cli_parse_superpixel_anywhere_in_argv():
    from drs_amd import cli
    got, value = cli.parse_superpixel(ARGV)
    assert value is None and got == ARGV and got is not ARGV
    assert cli.parse_superpixel(["--superpixel-vote"] + ARGV) == (ARGV, P.SuperpixelParams(8, 10, 5, "labels"))
    assert cli.parse_superpixel(["x.py", "--superpixel-weight=confidence", "a", "--superpixel-vote=16,20", "b"]) == (
        ARGV, P.SuperpixelParams(16, 20, 5, "confidence"))
    assert cli.parse_superpixel(ARGV + ["--superpixel-vote=4,1,16", "--superpixel-weight=labels"]) == (ARGV, P.SuperpixelParams(4, 1, 16, "labels"))
    for bad, say in ((["--superpixel-vote="], "--superpixel-vote=: expected --superpixel-vote or --superpixel-vote=size[,compactness[,iters]]"),
                     (["--superpixel-vote", "--superpixel-vote=8"], "more than once"), (["--superpixel-vote=3"], "--superpixel-vote=3: expected"),
                     (["--superpixel-vote=8,10,5,1"], "--superpixel-vote=8,10,5,1: expected"), (["--superpixel-vote=x"], "--superpixel-vote=x: expected"),
                     (["--superpixel-vote=8,41"], "compactness 1..40"), (["--superpixel-weight=confidence"], "give --superpixel-vote as well"),
                     (["--superpixel-vote", "--superpixel-weight=posterior"], "--superpixel-weight=labels|confidence"),
                     (["--superpixel-vote", "--superpixel-weight"], "--superpixel-weight=labels|confidence"),
                     (["--superpixel-vote", "--superpixel-weight=labels", "--superpixel-weight=labels"], "more than once")):
        with pytest.raises(ValueError) as e:
            cli.parse_superpixel(ARGV + bad)
        assert say in str(e.value), (bad, str(e.value))


def test_cli_flag_without_a_map_making_run_exits():
    from drs_amd import cli
    from drs_amd.net import NoComm
    for tail, say in ((["training", "--superpixel-vote"], "--superpixel-vote applies to the validate_test and generate_final_maps processes only"),
                      (["validate_test", "--superpixel-vote=2"], "--superpixel-vote=2: expected"),
                      (["validate_test", "--superpixel-weight=confidence"], "give --superpixel-vote as well"),
                      (["generate_final_maps", "--superpixel-vote=8", "--superpixel-vote=8"], "more than once")):
        with pytest.raises(SystemExit) as e:
            cli.main(MAIN_ARGV + tail, device="cpu", comm=NoComm())
        assert say in str(e.value), (tail, str(e.value))
    assert "--superpixel-vote[=size[,compactness[,iters]]]" in cli.__doc__ and "--superpixel-weight=labels|confidence" in cli.__doc__


class _Reached(Exception):
    pass


@pytest.mark.parametrize("process", ["validate_test", "generate_final_maps"])
@pytest.mark.parametrize("flags, want", [([], "absent"), (["--superpixel-vote"], P.SuperpixelParams(8, 10, 5, "labels")),
                                         (["--superpixel-weight=confidence", "--sieve=9", "--superpixel-vote=16,5,2", "--crf"],
                                          P.SuperpixelParams(16, 5, 2, "confidence"))])
def test_cli_flag_reaches_the_loops(monkeypatch, tmp_path, process, flags, want):
    """main parses, loads the synthetic tiles and calls the loop with superpixel=...: the net and the checkpoint are stand-ins, the
    loop itself is intercepted.  Without the flag the loop is called without the argument at all."""
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
    monkeypatch.setattr(loops, process, loop)
    argv = list(MAIN_ARGV)
    argv[1], argv[2], argv[3] = "synthetic:30x32x5/vaihingen/", str(tmp_path) + "/", "model-7"
    with pytest.raises(_Reached):
        cli.main(argv + [process] + flags, device="cpu", comm=NoComm())
    assert seen.get("superpixel", "absent") == want
    assert ("crf" in seen) == ("--crf" in flags) and ("sieve" in seen) == ("--sieve=9" in flags)


def test_the_loops_refuse_a_bad_spec_before_they_touch_the_net():
    from drs_amd import loops
    with pytest.raises(ValueError, match="size 3"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, superpixel=3)
    with pytest.raises(ValueError, match="'posterior'"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, superpixel=dict(weight="posterior"))
    with pytest.raises(ValueError, match="iters 17"):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, superpixel=(8, 10, 17))


def test_superpixel_str():
    from drs_amd import loops
    a, b = {"regions": 30, "changed_pixels": 40, "centres": 25}, {"regions": 3, "changed_pixels": 2, "centres": 2}
    sp = P.SuperpixelParams(16, 20, 3, "confidence")
    assert loops._superpixel_str(sp, a) == "Superpixel size= 16 compactness= 20 iters= 3 weight= confidence Regions= 30 Changed Pixels= 40"
    assert loops._superpixel_str(sp, [a, b]) == "Superpixel size= 16 compactness= 20 iters= 3 weight= confidence Regions= 33 Changed Pixels= 42"


# ------------------------------------------------------------------------------------------------------------- the entry points' checks
OK, ERR_ARG, ERR_HIP = 0, 1, 2
p0, p1, p2, p3, p4, p5 = [0x10000 + 0x1000 * i for i in range(6)]         # dummy device pointers: host code never dereferences them
LO, INV = (C.c_float * 8)(*[0.0] * 8), (C.c_float * 8)(*[1.0] * 8)
SHAPE_BAD = [dict(h=0), dict(w=0), dict(h=-40), dict(w=-52), dict(h=32769), dict(w=32769), dict(h=1 << 20, w=1 << 20)]
C_BAD = [dict(C=0), dict(C=9), dict(C=-5)]
ROWS = {
    "drs_superpixel_features": ([("tile", p0), ("tile_is_f64", 0), ("C", 5), ("h", 40), ("w", 52), ("lo", LO), ("inv", INV), ("feat", p1)],
                                SHAPE_BAD + C_BAD + [dict(tile_is_f64=2), dict(tile_is_f64=-1)]),
    "drs_superpixels": ([("feat", p0), ("C", 5), ("h", 40), ("w", 52), ("S", 8), ("m", 10), ("iters", 5), ("assign", p1), ("colour", p2),
                         ("centres", p3), ("scratch", p4)],
                        SHAPE_BAD + C_BAD + [dict(S=3), dict(S=33), dict(S=0), dict(S=-8), dict(m=0), dict(m=41), dict(m=-10), dict(iters=0),
                                             dict(iters=17), dict(iters=-5)]),
    "drs_region_vote": ([("map_in", p0), ("label", p1), ("weight", p2), ("h", 40), ("w", 52), ("K", 6), ("scratch", p3), ("map_out", p4),
                         ("counters", p5)],
                        SHAPE_BAD + [dict(K=0), dict(K=33), dict(K=-6)]),
}
MAY_BE_NULL = {"weight"}


def _call(lib, name, args, change=None):
    a = dict(args)
    a.update(change or {})
    return getattr(lib, name)(*[a[k] for k, _ in args], None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the baseline rows would launch kernels on dummy pointers: CPU machines only")
@pytest.mark.parametrize("name", sorted(ROWS))
def test_abi_rows(name):
    """in the manner of tests/test_abi_contract.py: the baseline is inside the domain (what comes back is the launch's status), every
    single-argument violation and every NULL pointer that may not be NULL returns exactly DRS_ERR_ARG"""
    from drs_amd import _lib
    lib = _lib.load()
    args, bad = ROWS[name]
    rc = _call(lib, name, args)
    assert rc != ERR_ARG and rc in (OK, ERR_HIP), (name, rc)
    nulls = [{k: None} for k, v in args if k not in MAY_BE_NULL and ((isinstance(v, int) and v >= 0x10000) or isinstance(v, C.Array))]
    assert len(nulls) >= 4
    wrong = [(change, rc) for change in bad + nulls for rc in [_call(lib, name, args, change)] if rc != ERR_ARG]
    assert not wrong, "%s: not DRS_ERR_ARG for %r" % (name, wrong)
    if name == "drs_region_vote":
        rc = _call(lib, name, args, dict(weight=None))
        assert rc != ERR_ARG and rc in (OK, ERR_HIP)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a missing check would launch kernels on dummy pointers: CPU machines only")
def test_lo_and_inv_are_not_read_before_C_is_checked():
    from drs_amd import _lib
    lib = _lib.load()
    one = (C.c_float * 1)(0.0)
    assert _call(lib, "drs_superpixel_features", ROWS["drs_superpixel_features"][0], dict(C=9, lo=one, inv=one)) == ERR_ARG


def test_the_size_queries_are_pure_and_zero_outside_the_ranges():
    from drs_amd import _lib
    q = lambda *a: _lib.query("drs_superpixel_scratch_bytes", *a)
    assert q(5, 40, 52, 8) == 4 * 5 * 6 * 8 and q(1, 1, 1, 4) == 16 and q(8, 3, 3, 32) == 44
    assert q(8, 32768, 32768, 4) == 4 * 8192 * 8192 * 11 and q(3, 37, 53, 5) == 4 * 7 * 10 * 6
    for bad in ((0, 40, 52, 8), (9, 40, 52, 8), (5, 0, 52, 8), (5, 40, 0, 8), (5, -1, 52, 8), (5, 32769, 52, 8), (5, 40, 32769, 8),
                (5, 40, 52, 3), (5, 40, 52, 33)):
        assert q(*bad) == 0, bad
    v = lambda *a: _lib.query("drs_region_vote_scratch_bytes", *a)
    assert v(40, 52) == 16 * 40 * 52 and v(1, 1) == 16 and v(32768, 32768) == 16 << 30
    for h, w in ((0, 5), (5, 0), (-1, 5), (32769, 5), (5, 32769)):
        assert v(h, w) == 0
    for name in ("drs_superpixel_features", "drs_superpixel_scratch_bytes", "drs_superpixels", "drs_region_vote_scratch_bytes", "drs_region_vote"):
        assert name in _lib.SIGNATURES
