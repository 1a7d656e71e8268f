"""CPU: the host side of the sieve: the numpy statement of the components, the round, the sieve and the census
(tests/sieve_ref.py) that the device tests are held to, on maps worked by hand and on the device tests' inputs;
patches.check_sieve / parse_sieve, the command-line flags, and the argument checks of the four entry points (host code: no launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sieve_ref
from drs_amd import patches as P


def _u8(rows):
    return np.array(rows, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------- the reference itself
def test_ref_components_on_a_hand_worked_map():
    m = _u8([[0, 0, 1, 1],
             [0, 2, 2, 1],
             [3, 0, 2, 1]])
    label, size = sieve_ref.components(m, 4)
    np.testing.assert_array_equal(label, [[0, 0, 2, 2], [0, 5, 5, 2], [8, 9, 5, 2]])
    np.testing.assert_array_equal(size, [[3, 3, 4, 4], [3, 3, 3, 4], [1, 1, 3, 4]])
    assert label.dtype == np.int32 and size.dtype == np.uint32
    label, size = sieve_ref.components(m, 8)                               # the 0 at (2, 1) touches (1, 0) by a corner
    np.testing.assert_array_equal(label, [[0, 0, 2, 2], [0, 5, 5, 2], [8, 0, 5, 2]])
    np.testing.assert_array_equal(size, [[4, 4, 4, 4], [4, 3, 3, 4], [1, 4, 3, 4]])


def test_ref_diagonal_line_is_one_component_at_8_and_pixels_at_4():
    m = np.zeros((6, 6), dtype=np.uint8)
    m[np.arange(6), np.arange(6)] = 1
    l4, s4 = sieve_ref.components(m, 4)
    l8, s8 = sieve_ref.components(m, 8)
    d = np.arange(6)
    np.testing.assert_array_equal(l4[d, d], d * 7)
    assert (s4[d, d] == 1).all() and (l8[d, d] == 0).all() and (s8[d, d] == 6).all()
    # the two triangles of zeros beside the line: apart at 4; at 8 they touch by corners ACROSS the line, (0, 1)-(1, 0), and are one
    # component of 30 pixels
    assert s4[0, 1] == 15 == s4[1, 0] and l4[0, 1] == 1 and l4[1, 0] == 6
    assert s8[0, 1] == 30 == s8[1, 0] and l8[1, 0] == 1
    # so a sieve at 8 keeps the line where a sieve at 4 removes it
    out4, _ = sieve_ref.sieve(m, 2, 4, 4)
    out8, info8 = sieve_ref.sieve(m, 2, 4, 8)
    assert (out4 == 0).all() and (out8 == m).all() and info8["merged"] == 0 and info8["left_small"] == 0


def test_ref_components_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for m in (sieve_ref.speckled(45, 131, 6), sieve_ref.serpentine(67, 131), sieve_ref.noise()):
        for c, structure in ((4, None), (8, np.ones((3, 3)))):
            label, size = sieve_ref.components(m, c)
            count = 0
            for b in np.unique(m):
                lab, n = ndi.label(m == b, structure=structure)
                count += n
                for i in range(1, n + 1):
                    mine = lab == i
                    assert (label[mine] == np.flatnonzero(mine.reshape(-1))[0]).all() and (size[mine] == mine.sum()).all()
            assert len(np.unique(label)) == count


def test_ref_a_lone_pixel_merges_into_its_surroundings():
    m = np.zeros((5, 5), dtype=np.uint8)
    m[2, 2] = 1
    out, counters = sieve_ref.sieve_round(m, 2, 2, 4)
    assert (out == 0).all() and counters == [1, 1]
    out, info = sieve_ref.sieve(m, 2, 2, 4)
    assert (out == 0).all()
    assert info == {"rounds": 2, "merged": 1, "left_small": 0, "changed_pixels": 1, "objects_before": [1, 1], "objects_after": [1, 0],
                    "capped": False}
    # min_size 0 or 1: nothing is small
    for ms in (0, 1, (24, 1)):
        out, info = sieve_ref.sieve(m, 2, ms, 4)
        assert (out == m).all() and info["rounds"] == 1 and info["merged"] == 0 and info["left_small"] == 0


def test_ref_a_tie_goes_to_the_lower_byte_and_size_beats_byte():
    m = _u8([[2, 2, 2, 0, 1, 1, 1],
             [2, 2, 2, 3, 1, 1, 1]])                                       # 0 and 3 are single pixels between two regions of 6
    out, counters = sieve_ref.sieve_round(m, 4, (2, 2, 2, 2), 4)
    assert counters == [2, 2]
    assert out[0, 3] == 1 and out[1, 3] == 1                               # equal sizes: the lower byte, 1
    m2 = np.concatenate([m, _u8([[2, 2, 2, 2, 9, 9, 9]])])                 # the region of 2 now has 10 pixels and reaches under the 3
    out, _ = sieve_ref.sieve_round(m2, 4, (2, 2, 2, 2), 4)
    assert out[0, 3] == 2 and out[1, 3] == 2                               # the larger region wins whatever its byte


def test_ref_a_speck_touching_only_specks_waits_a_round():
    m = np.zeros((7, 7), dtype=np.uint8)
    m[2:5, 2:5] = 1                                                        # a ring of 8 pixels of 1 (small at 9) ...
    m[3, 3] = 2                                                            # ... around a single 2 that touches nothing else
    out, counters = sieve_ref.sieve_round(m, 3, 9, 4)
    assert counters == [2, 1] and out[3, 3] == 2 and (out[m == 1] == 0).all()
    out, counters = sieve_ref.sieve_round(out, 3, 9, 4)
    assert counters == [1, 1] and (out == 0).all()
    assert sieve_ref.sieve(m, 3, 9, 4)[1]["rounds"] == 3


def test_ref_a_byte_beyond_K_neither_changes_nor_spreads():
    m = np.full((6, 8), 7, dtype=np.uint8)                                 # a field of a byte >= K ...
    m[2, 3] = 1                                                            # ... holds a speck: no pair offers anything
    m[4, 1:3] = 9                                                          # and a small region of another byte >= K
    out, info = sieve_ref.sieve(m, 3, 5, 4)
    assert (out == m).all() and info["merged"] == 0 and info["left_small"] == 1 and info["objects_before"] == [0, 1, 0]
    m[0:3, 4:8] = 0                                                        # a region of 12 pixels of class 0 beside the speck
    out, info = sieve_ref.sieve(m, 3, 5, 4)
    assert out[2, 3] == 0 and (out[m >= 3] == m[m >= 3]).all() and info["merged"] == 1


def test_ref_census_bins_by_the_power_of_two():
    m = _u8([[0, 0, 0, 1], [0, 1, 1, 1], [2, 2, 2, 2], [5, 0, 0, 0]])
    label, size = sieve_ref.components(m, 4)
    table = sieve_ref.census(m, label, size, 3)
    assert table.shape == (3, 32) and table.dtype == np.int64 and table.sum() == 4        # the byte 5 is not counted
    assert table[0, 2] == 1 and table[0, 1] == 1 and table[1, 2] == 1 and table[2, 2] == 1  # sizes 4, 3, 4, 4


CASES = [("speckled-45x131-K6", sieve_ref.speckled(45, 131, 6), 6, 12), ("speckled-33x65-K8", sieve_ref.speckled(33, 65, 8), 8, (5, 0, 9, 3, 20, 7, 7, 2)),
         ("speckled-1x40", sieve_ref.speckled(1, 40, 3), 3, 4), ("speckled-40x1", sieve_ref.speckled(40, 1, 3), 3, 4),
         ("rings", sieve_ref.rings(), 3, 200), ("noise", sieve_ref.noise(), 4, 16)]


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name, m, K, min_size", CASES, ids=[x[0] for x in CASES])
def test_ref_invariants_on_the_device_tests_inputs(name, m, K, min_size, c):
    out, info = sieve_ref.sieve(m, K, min_size, c)
    assert not info["capped"] and 2 <= info["rounds"] < sieve_ref.SIEVE_MAX_ROUNDS and info["left_small"] == 0 and info["merged"] > 0
    label, size = sieve_ref.components(out, c)
    assert not sieve_ref.small_mask(out, size, K, min_size).any()
    assert sum(info["objects_after"]) < sum(info["objects_before"])
    again, info2 = sieve_ref.sieve(out, K, min_size, c)                    # idempotent
    assert (again == out).all() and info2["rounds"] == 1 and info2["merged"] == 0 and info2["changed_pixels"] == 0
    assert info2["objects_before"] == info["objects_after"] == info2["objects_after"]
    if name == "rings":
        assert info["rounds"] == 7 and info["merged"] == 6 and (out == 0).all()


def test_ref_a_map_without_any_non_small_component_comes_back_unchanged():
    m = sieve_ref.speckled(5, 7, 2)
    for c in (4, 8):
        out, info = sieve_ref.sieve(m, 2, 100, c)
        assert (out == m).all() and info["rounds"] == 1 and info["merged"] == 0 and info["left_small"] > 0 and not info["capped"]
    m = sieve_ref.checkerboard(67, 131)
    out, info = sieve_ref.sieve(m, 2, 2, 4)
    assert (out == m).all() and info["left_small"] == 67 * 131


def test_ref_cap_is_reported():
    out, info = sieve_ref.sieve(sieve_ref.rings(), 3, 200, 4, max_rounds=3)
    assert info["capped"] and info["rounds"] == 3 and info["merged"] == 3 and info["left_small"] == 3


# ------------------------------------------------------------------------------------------------------------- the option's values
def test_check_sieve_and_parse():
    assert P.SIEVE_MAX_ROUNDS == 64 == sieve_ref.SIEVE_MAX_ROUNDS and P.SIEVE_CONNECTIVITY == 4
    assert P.check_sieve(16) == P.SieveParams((16,), 4) == P.check_sieve(np.int64(16))
    assert P.check_sieve([1, 0, 3]) == P.SieveParams((1, 0, 3), 4) == P.check_sieve(np.array([1, 0, 3]))
    assert P.check_sieve(dict(min_size=(2, 2), connectivity=8)) == P.SieveParams((2, 2), 8)
    assert P.check_sieve(dict(min_size=5)) == P.SieveParams((5,), 4)
    got = P.check_sieve(P.SieveParams((np.int32(3), 4), np.int64(8)))
    assert got == ((3, 4), 8) and all(type(v) is int for v in got.min_size) and type(got.connectivity) is int
    assert P.check_sieve(0).min_size == (0,) and P.check_sieve(1 << 30).min_size == (1 << 30,)
    assert P.sieve_thresholds(P.check_sieve(7), 6) == (7,) * 6 and P.sieve_thresholds(P.check_sieve([1, 2]), 2) == (1, 2)
    assert P.parse_sieve("16") == (16,) and P.parse_sieve("32,32,8,32,4,0") == (32, 32, 8, 32, 4, 0)


@pytest.mark.parametrize("bad, names", [
    (-1, "-1"), ((1 << 30) + 1, str((1 << 30) + 1)), (1.5, "1.5"), (True, "True"), (None, "None"), ("16", "'16'"), ((), "()"), ([], "[]"),
    ((1, -2), "-2"), ((1, 2.0), "2.0"), ((1, "2"), "'2'"), (tuple(range(33)), "32"), (dict(min_size=3, connectivity=6), "6"),
    (dict(min_size=3, connectivity=True), "True"), (dict(connectivity=4), "min_size"), (dict(min_size=3, rounds=2), "'rounds'"),
    (dict(min_size=None), "None"),
])
def test_check_sieve_names_the_offender(bad, names):
    with pytest.raises(ValueError) as e:
        P.check_sieve(bad)
    assert names in str(e.value), str(e.value)


def test_sieve_thresholds_wants_one_or_K():
    with pytest.raises(ValueError, match="3 given, expected 1 or 6"):
        P.sieve_thresholds(P.check_sieve((1, 2, 3)), 6)
    with pytest.raises(ValueError, match="33"):
        P.sieve_thresholds(P.check_sieve(1), 33)


@pytest.mark.parametrize("bad", ["", "1.5", "1, 2", " 1", "1,", ",1", "a", "1,-2", "+1", "-1", str((1 << 30) + 1), None, 3])
def test_parse_sieve_refuses(bad):
    with pytest.raises(ValueError):
        P.parse_sieve(bad)


# ------------------------------------------------------------------------------------------------------------- the command line
ARGV = ["x.py", "a", "b"]
MAIN_ARGV = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
             "single_fixed", "25", "acc"]


def test_cli_parse_sieve_anywhere_in_argv():
    from drs_amd import cli
    got, value = cli.parse_sieve(ARGV)
    assert value is None and got == ARGV and got is not ARGV
    assert cli.parse_sieve(["--sieve=16"] + ARGV, 6) == (ARGV, P.SieveParams((16,), 4))
    assert cli.parse_sieve(["x.py", "--sieve-connectivity=8", "a", "--sieve=1,2,3,4,5,0", "b"], 6) == (ARGV, P.SieveParams((1, 2, 3, 4, 5, 0), 8))
    assert cli.parse_sieve(ARGV + ["--sieve=1,2"]) == (ARGV, P.SieveParams((1, 2), 4))           # no class count given: any count
    for bad, say in ((["--sieve"], "--sieve=N or --sieve=n0,n1,..."), (["--sieve="], "--sieve=N or --sieve=n0,n1,..."),
                     (["--sieve=4", "--sieve=4"], "more than once"), (["--sieve=1,2"], "2 thresholds given, expected"),
                     (["--sieve=1,2,3,4,5,6,7"], "7 thresholds given"), (["--sieve=x"], "--sieve=x: expected"),
                     (["--sieve=-3"], "--sieve=-3: expected"), (["--sieve-connectivity=8"], "give --sieve as well"),
                     (["--sieve=4", "--sieve-connectivity=6"], "--sieve-connectivity=4|8"),
                     (["--sieve=4", "--sieve-connectivity"], "--sieve-connectivity=4|8"),
                     (["--sieve=4", "--sieve-connectivity=4", "--sieve-connectivity=8"], "more than once")):
        with pytest.raises(ValueError) as e:
            cli.parse_sieve(ARGV + bad, 6)
        assert say in str(e.value), (bad, str(e.value))


def test_cli_flag_without_a_map_making_run_exits():
    from drs_amd import cli
    from drs_amd.net import NoComm
    for tail, say in ((["training", "--sieve=16"], "--sieve applies to the validate_test and generate_final_maps processes only"),
                      (["validate_test", "--sieve=1,2,3"], "3 thresholds given, expected"),
                      (["validate_test", "--sieve-connectivity=8"], "give --sieve as well"),
                      (["generate_final_maps", "--sieve=8", "--sieve=8"], "more than once")):
        with pytest.raises(SystemExit) as e:
            cli.main(MAIN_ARGV + tail, device="cpu", comm=NoComm())
        assert say in str(e.value), (tail, str(e.value))


class _Reached(Exception):
    pass


@pytest.mark.parametrize("process", ["validate_test", "generate_final_maps"])
@pytest.mark.parametrize("flags, want", [([], "absent"), (["--sieve=16"], P.SieveParams((16,), 4)),
                                         (["--sieve=9,9,9,9,4,0", "--sieve-connectivity=8", "--crf"], P.SieveParams((9, 9, 9, 9, 4, 0), 8))])
def test_cli_flag_reaches_the_loops(monkeypatch, tmp_path, process, flags, want):
    """main parses, loads the synthetic tiles and calls the loop with sieve=...: the net and the checkpoint are stand-ins, the loop
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
    monkeypatch.setattr(loops, process, loop)
    argv = list(MAIN_ARGV)
    argv[1], argv[2], argv[3] = "synthetic:30x32x5/vaihingen/", str(tmp_path) + "/", "model-7"
    with pytest.raises(_Reached):
        cli.main(argv + [process] + flags, device="cpu", comm=NoComm())
    assert seen.get("sieve", "absent") == want
    assert ("crf" in seen) == ("--crf" in flags)


def test_the_loops_refuse_a_bad_sieve_before_they_touch_the_net():
    from drs_amd import loops
    with pytest.raises(ValueError, match="-5"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, sieve=-5)
    with pytest.raises(ValueError, match="connectivity 6"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, sieve=dict(min_size=4, connectivity=6))
    with pytest.raises(ValueError, match="sieve threshold"):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, sieve=(1, 2.5))


def test_sieve_str():
    from drs_amd import loops
    a = {"rounds": 3, "merged": 10, "left_small": 0, "changed_pixels": 40, "objects_before": [5, 7], "objects_after": [1, 2], "capped": False}
    b = {"rounds": 2, "merged": 1, "left_small": 0, "changed_pixels": 2, "objects_before": [1, 1], "objects_after": [1, 0], "capped": False}
    sv = P.SieveParams((16, 4), 8)
    assert loops._sieve_str(sv, a) == ("Sieve min= 16 4 connectivity= 8 Rounds= 3 Merged Components= 10 Changed Pixels= 40 "
                                       "Objects per class= [5 7] -> [1 2]")
    assert loops._sieve_str(sv, [a, b]) == ("Sieve min= 16 4 connectivity= 8 Rounds= 3 Merged Components= 11 Changed Pixels= 42 "
                                            "Objects per class= [6 8] -> [2 2]")


# ------------------------------------------------------------------------------------------------------------- the entry points' checks
OK, ERR_ARG, ERR_HIP = 0, 1, 2
p0, p1, p2, p3, p4, p5 = [0x10000 + 0x1000 * i for i in range(6)]         # dummy device pointers: host code never dereferences them
MIN6 = (C.c_int * 6)(16, 16, 4, 16, 0, 1 << 30)
MIN_NEG = (C.c_int * 6)(16, 16, 4, 16, -1, 16)
MIN_BIG = (C.c_int * 6)(16, 16, 4, 16, 0, (1 << 30) + 1)
SHAPE_BAD = [dict(h=0), dict(w=0), dict(h=-40), dict(w=-52), dict(h=1 << 16, w=(1 << 14) + 1), dict(h=1 << 20, w=1 << 20)]
ROWS = {
    "drs_components": ([("map", p0), ("h", 40), ("w", 52), ("connectivity", 4), ("label", p1), ("size", p2)],
                       SHAPE_BAD + [dict(connectivity=0), dict(connectivity=6), dict(connectivity=-4), dict(connectivity=16)]),
    "drs_sieve_round": ([("map_in", p0), ("label", p1), ("size", p2), ("h", 40), ("w", 52), ("K", 6), ("min_size", MIN6), ("scratch", p3),
                         ("map_out", p4), ("counters", p5)],
                        SHAPE_BAD + [dict(K=0), dict(K=33), dict(K=-6), dict(min_size=MIN_NEG), dict(min_size=MIN_BIG)]),
    "drs_component_census": ([("map", p0), ("label", p1), ("size", p2), ("h", 40), ("w", 52), ("K", 6), ("table", p3)],
                             SHAPE_BAD + [dict(K=0), dict(K=33), dict(K=-6)]),
}


def _call(lib, name, args, change=None):
    a = dict(args)
    a.update(change or {})
    return getattr(lib, name)(*[a[k] for k, _ in args], None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the baseline rows would launch kernels on dummy pointers: CPU machines only")
@pytest.mark.parametrize("name", sorted(ROWS))
def test_abi_rows(name):
    """in the manner of tests/test_abi_contract.py: the baseline is inside the domain (what comes back is the launch's status), every
    single-argument violation and every NULL pointer returns exactly DRS_ERR_ARG"""
    from drs_amd import _lib
    lib = _lib.load()
    args, bad = ROWS[name]
    rc = _call(lib, name, args)
    assert rc != ERR_ARG and rc in (OK, ERR_HIP), (name, rc)
    nulls = [{k: None} for k, v in args if (isinstance(v, int) and v >= 0x10000) or isinstance(v, C.Array)]
    assert len(nulls) >= 3
    wrong = [(change, rc) for change in bad + nulls for rc in [_call(lib, name, args, change)] if rc != ERR_ARG]
    assert not wrong, "%s: not DRS_ERR_ARG for %r" % (name, wrong)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a missing check would launch kernels on dummy pointers: CPU machines only")
def test_min_size_is_not_read_before_K_is_checked():
    from drs_amd import _lib
    lib = _lib.load()
    # a K beyond the array does not walk off it
    assert _call(lib, "drs_sieve_round", ROWS["drs_sieve_round"][0], dict(K=33, min_size=(C.c_int * 1)(5))) == ERR_ARG


def test_scratch_bytes_is_a_pure_query():
    from drs_amd import _lib
    assert _lib.query("drs_sieve_scratch_bytes", 40, 52) == 8 * 40 * 52
    assert _lib.query("drs_sieve_scratch_bytes", 1 << 15, 1 << 15) == 8 << 30 and _lib.query("drs_sieve_scratch_bytes", 1, 1) == 8
    for h, w in ((0, 5), (5, 0), (-1, 5), (1 << 16, (1 << 14) + 1)):
        assert _lib.query("drs_sieve_scratch_bytes", h, w) == 0
    for name in ("drs_components", "drs_sieve_scratch_bytes", "drs_sieve_round", "drs_component_census"):
        assert name in _lib.SIGNATURES
