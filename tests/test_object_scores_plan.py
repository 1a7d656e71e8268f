"""CPU: the host side of the object scores: the numpy statement of the match and the table (tests/objects_ref.py) that
the device tests are held to, against an independent brute force and on the device tests' fixtures; metrics.object_scores on tables
worked by hand; patches.check_object_scores / parse_object_scores, the command-line flag, the argument checks of the three entry
points (host code: no launch), where the declarations sit, and that validate_test without the option is what it was."""
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import objects_ref
import sieve_ref
from drs_amd import patches as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- the reference itself
def _brute(truth, pred, K, ignore, c):
    """every (truth object, predicted object) pair, objects as pixel sets, IoU as a Fraction: {t root: (p root, I)} of the pairs with
    IoU > 1/2, cover per predicted root, and the table"""
    h, w = truth.shape
    tl, _ = sieve_ref.components(truth, c)
    pl, _ = sieve_ref.components(pred, c)
    counted = {(y, x) for y in range(h) for x in range(w) if truth[y, x] != ignore and truth[y, x] < K}
    tobj, pobj = {}, {}
    for y in range(h):
        for x in range(w):
            if (y, x) in counted:
                tobj.setdefault(int(tl[y, x]), set()).add((y, x))
            if pred[y, x] < K:
                pobj.setdefault(int(pl[y, x]), set()).add((y, x))
    byte = lambda m, r: int(m.reshape(-1)[r])
    cover = {p: len(s & counted) for p, s in pobj.items()}
    found = {}
    for t, ts in tobj.items():
        for p, ps in pobj.items():
            if byte(truth, t) != byte(pred, p):
                continue
            I = len(ts & ps)
            union = len(ts) + cover[p] - I
            if union and Fraction(I, union) > Fraction(1, 2):
                assert t not in found and p not in [q for q, _ in found.values()], "IoU > 1/2 matched an object twice"
                found[t] = (p, I)
    table = np.zeros((K, 4, 32), dtype=np.int64)
    for t, ts in tobj.items():
        b = int(math.floor(math.log2(len(ts))))
        table[byte(truth, t), 0, b] += 1
        if t in found:
            p, I = found[t]
            table[byte(truth, t), 2, b] += 1
            table[byte(truth, t), 3, b] += int(Fraction(I, len(ts) + cover[p] - I) * (1 << 20))
    taken = {p for p, _ in found.values()}
    for p, ps in pobj.items():
        if p in taken or 2 * cover[p] >= len(ps):
            table[byte(pred, p), 1, int(math.floor(math.log2(len(ps))))] += 1
    return found, cover, table


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("seed", range(6))
def test_ref_against_brute_force_on_small_maps_with_an_ignore_band(seed, c):
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(3, 13)), int(rng.integers(3, 13))
    K = 3
    truth = sieve_ref.speckled(h, w, K, seed=seed, frac=0.1)
    pred = objects_ref.flipped(truth, K, frac=0.15, seed=seed + 50)
    pred[rng.random((h, w)) < 0.05] = 5                                    # bytes >= K in the prediction
    x0 = int(rng.integers(0, w - 1))
    truth = objects_ref.with_band(truth, x0, x0 + 2, byte=6)               # the ignore band
    if seed % 2:
        truth[0, 0] = 4                                                    # a truth byte >= K that is not the ignore label
    m, inter, cover, (tl, ts, pl, ps) = objects_ref.match(truth, pred, K, 6, c)
    found, bcover, btable = _brute(truth, pred, K, 6, c)
    idx = np.arange(h * w)
    troots = set(idx[(tl == idx) & objects_ref.counted_mask(truth.reshape(-1), K, 6)].tolist())
    for i in range(h * w):
        if i in troots:
            assert (int(m[i]), int(inter[i])) == (found[i] if i in found else (-1, 0)), i
        else:
            assert m[i] == -2 and inter[i] == 0
        assert cover[i] == bcover.get(i, 0)
    np.testing.assert_array_equal(objects_ref.table(truth, pred, K, 6, c), btable)


def test_ref_hand_worked_cases():
    t, p2, p3 = objects_ref.half_cases()
    m, inter, cover, _ = objects_ref.match(t, p2, 2, -1, 4)
    r = 2 * 8 + 2                                                          # the root of the object and of both predictions
    assert m[r] == -1 and inter[r] == 0 and cover[r] == 2                  # IoU exactly 1/2: 3 I = 6 = |t| + cover
    m, inter, cover, _ = objects_ref.match(t, p3, 2, -1, 4)
    assert m[r] == r and inter[r] == 3 and cover[r] == 3                   # 9 > 7
    tab = objects_ref.table(t, p3, 2, -1, 4)
    assert tab[1, 0, 2] == 1 and tab[1, 1, 1] == 1 and tab[1, 2, 2] == 1 and tab[1, 3, 2] == (3 << 20) // 4
    t, p = objects_ref.swallowed()
    m, inter, cover, _ = objects_ref.match(t, p, 2, -1, 4)
    assert m[2 * 12 + 2] == -1 and inter[2 * 12 + 2] == 0 and cover[1 * 12 + 1] == 40
    t, p = objects_ref.fifths()
    m, inter, cover, _ = objects_ref.match(t, p, 2, -1, 4)
    assert m[46 + 1] == -1 and inter[46 + 1] == 0 and sorted(cover[cover > 0].tolist())[:5] == [200] * 5
    t, p = objects_ref.band_case()
    tab = objects_ref.table(t, p, 6, 6, 4)
    # class 1: three truth objects (80, 16, 24 pixels), two found; predicted: A (false positive), C and D (matched; D although most of
    # it lies in the band), B dropped
    assert tab[1, 0].sum() == 3 and tab[1, 2].sum() == 2 and tab[1, 1].sum() == 3
    assert tab[1, 3, 6] == 1 << 20 and tab[1, 3, 4] == 1 << 20             # both matches at IoU 1: the band's pixels do not count against them
    assert tab[1, 1, 5] == 1 and tab[1, 1, 6] == 1 and tab[1, 1, 7] == 1      # D (40) by its own size, A (72), C (128); B (84) nowhere


@pytest.mark.parametrize("name", sorted(objects_ref.fixtures()))
def test_fixtures_exercise_their_branches(name):
    """the condition on the device tests' fixtures: every multi-object fixture has a match, an unmatched truth object, an unmatched
    counted predicted object and, with an ignore band, a dropped predicted object"""
    truth, pred, K, ignore, multi = objects_ref.fixtures()[name]
    assert truth.shape == pred.shape and truth.dtype == pred.dtype == np.uint8
    for c in (4, 8):
        b = objects_ref.branches(truth, pred, K, ignore, c)
        if multi:
            assert b["matched"] > 0 and b["unmatched_truth"] > 0 and b["unmatched_pred"] > 0, (name, c, b)
            if ignore >= 0:
                assert b["dropped_pred"] > 0, (name, c, b)
    m, inter, cover, (tl, ts, pl, ps) = objects_ref.match(truth, pred, K, ignore, 4)
    if name == "holed-300x300":
        assert ts[0] == 90000 and m[0] == 0 and inter[0] == 90000 - 3600 > 65535
    if name == "serpentine-cut":
        corridor = int(truth.sum())
        assert m[0] == 0 and corridor / 2 < inter[0] < corridor and (pl[truth.reshape(-1) == 1] != 0).sum() > 1000
    if name == "fifths":
        assert m[46 + 1] == -1
    if name == "beyond-K":
        assert (pred >= K).sum() > 100 and (cover[pred.reshape(-1) >= K] == 0).all()


# ------------------------------------------------------------------------------------------------------------- the scores
def test_object_scores_on_hand_computed_tables():
    from drs_amd import metrics as MT
    t = np.zeros((4, 4, 32), dtype=np.int64)
    # class 0: 5 truth objects (3 of size 4..7, 2 of size 64..127), 4 predicted, 3 matched (2 small, 1 large) at IoU 0.75, 1.0, 0.6
    t[0, 0, 2], t[0, 0, 6] = 3, 2
    t[0, 1, 2], t[0, 1, 6] = 3, 1
    t[0, 2, 2], t[0, 2, 6] = 2, 1
    t[0, 3, 2], t[0, 3, 6] = (3 << 18) + (1 << 20), (3 << 20) // 5
    # class 1: present, nothing matched: 2 truth objects, 1 predicted.  class 2: absent.  class 3: predicted only
    t[1, 0, 0], t[1, 1, 3] = 2, 1
    t[3, 1, 10] = 7
    o = MT.object_scores(t)
    assert o["truth"].tolist() == [5, 2, 0, 0] and o["predicted"].tolist() == [4, 1, 0, 7] and o["matched"].tolist() == [3, 0, 0, 0]
    assert o["present"].tolist() == [True, True, False, True]
    assert o["precision"][0] == 0.75 and o["recall"][0] == 0.6 and o["f1"][0] == pytest.approx(6.0 / 9.0)
    sq0 = ((3 << 18) + (1 << 20) + (3 << 20) // 5) / (3 * 2.0 ** 20)
    assert o["sq"][0] == pytest.approx(sq0, abs=1e-15) and abs(sq0 - (0.75 + 1.0 + 0.6) / 3) < 1e-6
    assert o["pq"][0] == pytest.approx(sq0 * 6.0 / 9.0)
    # TP = 0 in a present class: F1 0, PQ 0, no SQ; a class without truth objects has no recall, one without predictions no precision
    assert o["f1"][1] == 0.0 and o["pq"][1] == 0.0 and math.isnan(o["sq"][1]) and o["precision"][1] == 0.0 and o["recall"][1] == 0.0
    assert o["f1"][3] == 0.0 and o["pq"][3] == 0.0 and math.isnan(o["recall"][3]) and o["precision"][3] == 0.0
    assert all(math.isnan(o[k][2]) for k in ("precision", "recall", "f1", "sq", "pq"))      # the absent class
    assert o["mean_f1"] == pytest.approx((6.0 / 9.0) / 3) and o["mean_pq"] == pytest.approx(sq0 * (6.0 / 9.0) / 3) and o["mean_sq"] == pytest.approx(sq0)
    assert o["mean_recall"] == pytest.approx(0.3) and o["mean_precision"] == pytest.approx(0.25)
    assert o["recall_by_size"][0, 2] == pytest.approx(2 / 3) and o["recall_by_size"][0, 6] == 0.5 and o["recall_by_size"][1, 0] == 0.0
    assert math.isnan(o["recall_by_size"][0, 3]) and o["recall_by_size"].shape == (4, 32)
    a = o["all"]
    assert (a["truth"], a["predicted"], a["matched"]) == (7, 12, 3) and a["f1"] == pytest.approx(6.0 / (6 + 9 + 4)) and a["sq"] == pytest.approx(sq0)
    # the restatement in the reference agrees
    per, whole = objects_ref.scores(t)
    for k in range(4):
        for key in ("precision", "recall", "f1", "sq", "pq"):
            assert (math.isnan(per[k][key]) and math.isnan(o[key][k])) or per[k][key] == pytest.approx(float(o[key][k]), abs=1e-15), (k, key)
    assert whole["pq"] == pytest.approx(a["pq"])
    empty = MT.object_scores(np.zeros((2, 4, 32), dtype=np.int64))
    assert empty["mean_pq"] == 0.0 and not empty["present"].any() and math.isnan(empty["all"]["f1"])


@pytest.mark.parametrize("bad", [np.zeros((3, 32), dtype=np.int64), np.zeros((3, 4, 31), dtype=np.int64), np.zeros((3, 4, 32)),
                                 -np.ones((1, 4, 32), dtype=np.int64), np.zeros((0, 4, 32), dtype=np.int64)])
def test_object_scores_refuses_another_table(bad):
    from drs_amd import metrics as MT
    with pytest.raises(ValueError, match="object table"):
        MT.object_scores(bad)


def test_object_scores_refuses_more_matches_than_objects():
    from drs_amd import metrics as MT
    t = np.zeros((1, 4, 32), dtype=np.int64)
    t[0, 2, 3] = 1
    with pytest.raises(ValueError, match="more matched"):
        MT.object_scores(t)


def test_objects_str():
    from drs_amd import loops, metrics as MT
    t = np.zeros((2, 4, 32), dtype=np.int64)
    t[0, 0, 3], t[0, 1, 3], t[0, 2, 3], t[0, 3, 3] = 2, 1, 1, 1 << 19
    line = loops._objects_str(8, MT.object_scores(t))
    assert line == ("Objects connectivity= 8 Truth= [2 0] Predicted= [1 0] Matched= [1 0] Precision= [1.000000 nan] Recall= [0.500000 nan] "
                    "F1= [0.666667 nan] SQ= [0.500000 nan] PQ= [0.333333 nan] Mean F1= 0.666667 Mean SQ= 0.500000 Mean PQ= 0.333333 "
                    "All Objects F1= 0.666667 SQ= 0.500000 PQ= 0.333333")


# ------------------------------------------------------------------------------------------------------------- the option's values
def test_check_and_parse_object_scores():
    assert P.OBJECT_CONNECTIVITY == 4
    assert P.check_object_scores(4) == 4 and P.check_object_scores(np.int64(8)) == 8 and type(P.check_object_scores(np.int32(8))) is int
    assert P.parse_object_scores("4") == 4 and P.parse_object_scores("8") == 8


@pytest.mark.parametrize("bad", [0, 6, -4, 16, True, None, "4", 4.0, (4,)])
def test_check_object_scores_names_the_offender(bad):
    with pytest.raises(ValueError) as e:
        P.check_object_scores(bad)
    assert repr(bad) in str(e.value)


@pytest.mark.parametrize("bad", ["", "6", " 4", "4 ", "4,8", "+4", "04", "x", None, 4])
def test_parse_object_scores_refuses(bad):
    with pytest.raises(ValueError):
        P.parse_object_scores(bad)


# ------------------------------------------------------------------------------------------------------------- the command line
ARGV = ["x.py", "a", "b"]
MAIN_ARGV = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
             "single_fixed", "25", "acc"]


def test_cli_parse_object_scores_anywhere_in_argv():
    from drs_amd import cli
    got, value = cli.parse_object_scores(ARGV)
    assert value is None and got == ARGV and got is not ARGV
    assert cli.parse_object_scores(["--object-scores"] + ARGV) == (ARGV, 4)
    assert cli.parse_object_scores(["x.py", "a", "--object-scores=8", "b"]) == (ARGV, 8)
    assert cli.parse_object_scores(ARGV + ["--object-scores=4"]) == (ARGV, 4)
    for bad, say in ((["--object-scores="], "--object-scores=: expected --object-scores or --object-scores=4|8"),
                     (["--object-scores=6"], "--object-scores=6: expected --object-scores or --object-scores=4|8"),
                     (["--object-scores=4,8"], "expected --object-scores or"),
                     (["--object-scores", "--object-scores=8"], "--object-scores given more than once")):
        with pytest.raises(ValueError) as e:
            cli.parse_object_scores(ARGV + bad)
        assert say in str(e.value), (bad, str(e.value))


def test_cli_flag_outside_validate_test_exits():
    from drs_amd import cli
    from drs_amd.net import NoComm
    for tail, say in ((["training", "--object-scores"], "--object-scores applies to the validate_test process only"),
                      (["generate_final_maps", "--object-scores=8"], "--object-scores applies to the validate_test process only"),
                      (["validate_test", "--object-scores=5"], "expected --object-scores or --object-scores=4|8"),
                      (["validate_test", "--object-scores", "--object-scores"], "more than once")):
        with pytest.raises(SystemExit) as e:
            cli.main(MAIN_ARGV + tail, device="cpu", comm=NoComm())
        assert say in str(e.value), (tail, str(e.value))


class _Reached(Exception):
    pass


@pytest.mark.parametrize("flags, want", [([], "absent"), (["--object-scores"], 4), (["--object-scores=8", "--sieve=16", "--crf"], 8)])
def test_cli_flag_reaches_validate_test(monkeypatch, tmp_path, flags, want):
    """main parses, loads the synthetic tiles and calls the loop with object_scores=...: the net and the checkpoint are stand-ins, the
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
    monkeypatch.setattr(loops, "validate_test", loop)
    argv = list(MAIN_ARGV)
    argv[1], argv[2], argv[3] = "synthetic:30x32x5/vaihingen/", str(tmp_path) + "/", "model-7"
    with pytest.raises(_Reached):
        cli.main(argv + ["validate_test"] + flags, device="cpu", comm=NoComm())
    assert seen.get("object_scores", "absent") == want
    assert ("sieve" in seen) == ("--sieve=16" in flags)


def test_the_other_flavours_do_not_take_the_flag():
    from drs_amd import cli
    src = inspect.getsource(cli)
    assert src.count("parse_object_scores(argv)") == 2                     # its definition and the isprs main
    assert 'OBJECT_SCORES_FLAG + " applies to the validate_test process only"' in src


def test_validate_test_without_the_option_is_what_it_was():
    """plan level: the option is keyword-only in effect (last, default None), refused before the net is touched, and everything it
    adds to validate_test sits behind `oconn is not None`; generate_final_maps does not know it"""
    from drs_amd import loops
    params = list(inspect.signature(loops.validate_test).parameters)
    assert params[-1] == "object_scores" and inspect.signature(loops.validate_test).parameters["object_scores"].default is None
    assert "object_scores" not in inspect.signature(loops.generate_final_maps).parameters
    with pytest.raises(ValueError, match="connectivity 6"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, object_scores=6)
    with pytest.raises(ValueError, match="True"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, object_scores=True)
    lines = inspect.getsource(loops.validate_test).split('"""', 2)[2].splitlines()
    mine = [i for i, line in enumerate(lines) if re.search(r"\bobject_table\(|_objects_str\(|all_otable|object_list|MT\.object_scores", line)]
    assert len(mine) >= 8
    for i in mine:
        indent = len(lines[i]) - len(lines[i].lstrip())
        last = {}
        for j, ln in enumerate(lines[:i]):                                 # the innermost enclosing `if` of every shallower indent
            ind = len(ln) - len(ln.lstrip())
            if ln.strip() and ind < indent:
                last = {k: v for k, v in last.items() if k < ind}
                if ln.strip().startswith("if "):
                    last[ind] = ln.strip()
        assert any("oconn is not None" in g for g in last.values()), lines[i]
    assert "oconn = None if object_scores is None else P.check_object_scores(object_scores)" in "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------- the entry points' checks
OK, ERR_ARG, ERR_HIP = 0, 1, 2
p0, p1, p2, p3, p4, p5, p6, p7, p8, p9 = [0x10000 + 0x1000 * i for i in range(10)]     # dummy device pointers: host code never dereferences them
SHAPE_BAD = [dict(h=0), dict(w=0), dict(h=-40), dict(w=-52), dict(h=1 << 16, w=(1 << 14) + 1), dict(h=1 << 20, w=1 << 20)]
DOMAIN_BAD = SHAPE_BAD + [dict(K=0), dict(K=33), dict(K=-6), dict(ignore_label=-2), dict(ignore_label=256), dict(ignore_label=-(1 << 31))]
ROWS = {
    "drs_object_match": ([("truth", p0), ("pred", p1), ("tlabel", p2), ("tsize", p3), ("plabel", p4), ("psize", p5), ("h", 40), ("w", 52),
                          ("K", 6), ("ignore_label", 6), ("scratch", p6), ("match", p7), ("inter", p8), ("cover", p9)], DOMAIN_BAD),
    "drs_object_table": ([("truth", p0), ("tlabel", p2), ("tsize", p3), ("pred", p1), ("plabel", p4), ("psize", p5), ("match", p7),
                          ("inter", p8), ("cover", p9), ("h", 40), ("w", 52), ("K", 6), ("ignore_label", -1), ("table", p6)], DOMAIN_BAD),
}


def _call(lib, name, args, change=None):
    a = dict(args)
    a.update(change or {})
    return getattr(lib, name)(*[a[k] for k, _ in args], None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the baseline rows would launch kernels on dummy pointers: CPU machines only")
@pytest.mark.parametrize("name", sorted(ROWS))
def test_abi_rows(name):
    """in the manner of tests/test_sieve_plan.py: the baseline is inside the domain (what comes back is the launch's status), every
    single-argument violation and every NULL pointer returns exactly DRS_ERR_ARG"""
    from drs_amd import _lib
    lib = _lib.load()
    args, bad = ROWS[name]
    rc = _call(lib, name, args)
    assert rc != ERR_ARG and rc in (OK, ERR_HIP), (name, rc)
    for edge in (dict(ignore_label=-1), dict(ignore_label=255), dict(K=1), dict(K=32), dict(h=1, w=1), dict(h=1 << 15, w=1 << 15)):
        assert _call(lib, name, args, edge) != ERR_ARG, (name, edge)
    nulls = [{k: None} for k, v in args if isinstance(v, int) and v >= 0x10000]
    assert len(nulls) == 10
    wrong = [(change, rc) for change in bad + nulls for rc in [_call(lib, name, args, change)] if rc != ERR_ARG]
    assert not wrong, "%s: not DRS_ERR_ARG for %r" % (name, wrong)


def test_scratch_bytes_is_a_pure_query():
    from drs_amd import _lib
    assert _lib.query("drs_object_scratch_bytes", 40, 52) == 8 * 40 * 52
    assert _lib.query("drs_object_scratch_bytes", 1 << 15, 1 << 15) == 8 << 30 and _lib.query("drs_object_scratch_bytes", 1, 1) == 8
    for h, w in ((0, 5), (5, 0), (-1, 5), (1 << 16, (1 << 14) + 1)):
        assert _lib.query("drs_object_scratch_bytes", h, w) == 0
    for _ in range(2):                                                     # the same answer every time: nothing is remembered
        assert _lib.query("drs_object_scratch_bytes", 6000, 6000) == 8 * 6000 * 6000


def test_the_declarations_sit_in_the_whole_map_section():
    import subprocess
    from drs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    names = ("drs_object_scratch_bytes", "drs_object_match", "drs_object_table")
    step = hdr.index("Step level: the reference's three `sess.run` call shapes")
    at = [hdr.index("int drs_component_census(")] + [re.search(r"^(?:int|size_t)\s+" + n + r"\s*\(", hdr, flags=re.M).start() for n in names]
    assert step < hdr.index("Whole-map level") < at[0] < at[1] < at[2] < at[3] < hdr.index("Training level: boundary-weighted") < hdr.index(
        "int drs_patch_boundary_weight(")
    # nothing is declared between the census and the three
    between = hdr[at[0]:at[1]]
    assert len(re.findall(r"^(?:int|void|float|long long|size_t)\s+drs_", between, flags=re.M)) == 1
    for text in ("3 I > |t| + cover(p)", "2 cover(p) >= |p|", "floor(I 2^20 / (|t| + cover(p) - I))", "tests/objects_ref.py", "DESIGN.md 8a.9"):
        assert text in hdr[at[0]:at[1]], text
    exported = set(re.findall(r" T (drs_[a-z0-9_]+)$", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                                                                        text=True, check=True).stdout, flags=re.M))
    lib = _lib.load()
    for name in names:
        m = re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\);", hdr, flags=re.M)
        nargs = len([a for a in m.group(1).replace("\n", " ").split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, (name, nargs)
        assert name in exported and hasattr(lib, name)
