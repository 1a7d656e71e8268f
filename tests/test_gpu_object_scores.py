"""-m gpu: the match of two component labellings and the object table (include/drs.h drs_object_match /
drs_object_table; loops.object_table, validate_test's object_scores) against their numpy statement tests/objects_ref.py.

Every comparison is exact integer equality: the rule is integer arithmetic, there are no tolerances and no excluded pixels."""
import numpy as np
import pytest
import torch

import objects_ref

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

# the tile of the kernels is 32 x 32.  objects_ref.fixtures: maps ragged against it in both axes with many matches and misses (flipped,
# shifted, with an ignore band, K 8, bytes >= K); one-pixel-wide maps and one smaller than a tile; one pair above 65 535 pixels whose
# votes all land on one word; a corridor whose majority only exists across many tiles; an object without a majority partner; IoU
# exactly 1/2 and just above; a partner that is too large; an ignore band that cuts predicted objects
FIXTURES = objects_ref.fixtures()
_REF = {}


def _ref(name, c):
    """the reference outputs of a fixture, computed once and shared by the tests (read-only)"""
    if (name, c) not in _REF:
        truth, pred, K, ignore, _ = FIXTURES[name]
        m, inter, cover, labels = objects_ref.match(truth, pred, K, ignore, c)
        table = objects_ref.table_from(truth, pred, K, ignore, m, inter, cover, labels)
        for a in (m, inter, cover, table):
            a.setflags(write=False)
        _REF[name, c] = (m, inter, cover, table)
    return _REF[name, c]


def _components(md, h, w, c):
    from drs_amd import _lib
    label = torch.full((h * w,), -7, dtype=torch.int32, device=DEV)
    size = torch.full((h * w,), -7, dtype=torch.int32, device=DEV)
    _lib.call("drs_components", md.data_ptr(), h, w, c, label.data_ptr(), size.data_ptr(), stream())
    return label, size


def _match(truth, pred, K, ignore, c, fill):
    """drs_components twice, drs_object_match with the scratch holding `fill`, drs_object_table twice into a table that holds
    something: (match, inter, cover as numpy, the table's increase halved)"""
    from drs_amd import _lib
    h, w = truth.shape
    n = h * w
    td, pd = dev(np.array(truth).reshape(-1)), dev(np.array(pred).reshape(-1))
    tlabel, tsize = _components(td, h, w, c)
    plabel, psize = _components(pd, h, w, c)
    nbytes = _lib.query("drs_object_scratch_bytes", h, w)
    assert nbytes == 8 * n
    scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    m = torch.full((n,), 12345, dtype=torch.int32, device=DEV)             # every element is stored: none of these survives
    inter = torch.full((n,), 12345, dtype=torch.int32, device=DEV)
    cover = torch.full((n,), 12345, dtype=torch.int32, device=DEV)
    _lib.call("drs_object_match", td.data_ptr(), pd.data_ptr(), tlabel.data_ptr(), tsize.data_ptr(), plabel.data_ptr(), psize.data_ptr(),
              h, w, K, ignore, scratch.data_ptr(), m.data_ptr(), inter.data_ptr(), cover.data_ptr(), stream())
    before = np.random.default_rng(1).integers(1, 1 << 40, size=(K, 4, 32), dtype=np.int64)    # the table is ADDED to
    table = dev(before.reshape(-1))
    for _ in range(2):
        _lib.call("drs_object_table", td.data_ptr(), tlabel.data_ptr(), tsize.data_ptr(), pd.data_ptr(), plabel.data_ptr(), psize.data_ptr(),
                  m.data_ptr(), inter.data_ptr(), cover.data_ptr(), h, w, K, ignore, table.data_ptr(), stream())
    torch.cuda.synchronize()
    grown = table.cpu().numpy().reshape(K, 4, 32) - before
    assert (grown % 2 == 0).all()
    return m.cpu().numpy(), inter.cpu().numpy().view(np.uint32), cover.cpu().numpy().view(np.uint32), grown // 2


# ------------------------------------------------------------------------------------------------------------- 1. match and table
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_match_and_table(name, c):
    truth, pred, K, ignore, _ = FIXTURES[name]
    want_m, want_inter, want_cover, want_table = _ref(name, c)
    first = None
    for fill in (0x00, 0xFF):                                              # the scratch holds zeros, then ones: the same bits
        m, inter, cover, table = _match(truth, pred, K, ignore, c, fill)
        np.testing.assert_array_equal(m, want_m, err_msg="match, fill=%#x" % fill)
        np.testing.assert_array_equal(inter, want_inter, err_msg="inter, fill=%#x" % fill)
        np.testing.assert_array_equal(cover, want_cover, err_msg="cover, fill=%#x" % fill)
        np.testing.assert_array_equal(table, want_table, err_msg="table, fill=%#x" % fill)
        if first is not None:
            assert all((a == b).all() for a, b in zip(first, (m, inter, cover, table)))
        first = (m, inter, cover, table)
    h, w = truth.shape
    if name == "holed-300x300":
        assert m[0] == 0 and inter[0] == 86400 and cover[0] == 86400 and (m >= 0).sum() == 1
    if name == "serpentine-cut":
        assert m[0] == 0 and inter[0] > truth.sum() // 2
    if name == "fifths":
        assert m[w + 1] == -1 and inter[w + 1] == 0
    if name == "half-exactly":
        assert m[2 * w + 2] == -1 and inter[2 * w + 2] == 0 and cover[2 * w + 2] == 2
    if name == "half-plus-one":
        assert m[2 * w + 2] == 2 * w + 2 and inter[2 * w + 2] == 3
    if name == "swallowed":
        assert m[2 * w + 2] == -1 and cover[w + 1] == 40
    if name == "band":
        assert table[1, 0].sum() == 3 and table[1, 2].sum() == 2 and table[1, 1, 5] == 1 and table[1, 1].sum() == 3


# ------------------------------------------------------------------------------------------------------------- 2. loops.object_table
def test_object_table_accumulates_two_maps_and_two_runs_give_the_same_bits():
    from drs_amd import loops, metrics as MT
    a, b = "speckled-flipped-band", "band"
    (ta, pa, K, ignore, _), (tb, pb, Kb, ignore_b, _) = FIXTURES[a], FIXTURES[b]
    assert K == Kb == 6 and ignore == ignore_b == 6
    for c in (4, 8):
        want = _ref(a, c)[3] + _ref(b, c)[3]
        table = loops.object_table(dev(np.array(ta)), dev(np.array(pa)), ta.shape[0], ta.shape[1], K, ignore, c)
        assert table.dtype == torch.int64 and tuple(table.shape) == (K, 4, 32)
        np.testing.assert_array_equal(table.cpu().numpy(), _ref(a, c)[3])
        same = loops.object_table(dev(np.array(tb)).reshape(-1), dev(np.array(pb)), tb.shape[0], tb.shape[1], K, ignore, c, table=table, stream=stream())
        torch.cuda.synchronize()
        assert same is table
        np.testing.assert_array_equal(table.cpu().numpy(), want)
        per, whole = objects_ref.scores(want)
        got = MT.object_scores(table.cpu().numpy())
        assert got["all"]["matched"] == whole["matched"] and got["all"]["pq"] == pytest.approx(whole["pq"], abs=1e-15)
    # no ignore label: None and -1 are the same
    t, p = FIXTURES["speckled-flipped"][:2]
    one = loops.object_table(dev(np.array(t)), dev(np.array(p)), 45, 131, 6, None, 4)
    two = loops.object_table(dev(np.array(t)), dev(np.array(p)), 45, 131, 6, -1, 4)
    assert torch.equal(one, two)
    with pytest.raises(ValueError, match="6"):
        loops.object_table(dev(np.array(t)), dev(np.array(p)), 45, 131, 6, -1, 6)
    with pytest.raises(ValueError, match="uint8"):
        loops.object_table(dev(np.array(t)).to(torch.int32), dev(np.array(p)), 45, 131, 6, -1, 4)
    with pytest.raises(ValueError, match=r"\[6\]\[4\]\[32\]"):
        loops.object_table(dev(np.array(t)), dev(np.array(p)), 45, 131, 6, -1, 4, table=torch.zeros((6, 32), dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------------------- 3. arguments
def test_rejected_arguments_launch_nothing():
    from drs_amd import _lib
    truth, pred = FIXTURES["speckled-5x7"][:2]
    td, pd = dev(np.array(truth).reshape(-1)), dev(np.array(pred).reshape(-1))
    tlabel, tsize = _components(td, 5, 7, 4)
    plabel, psize = _components(pd, 5, 7, 4)
    scratch = torch.zeros(35, dtype=torch.int64, device=DEV)
    m, inter, cover = [torch.full((35,), 77, dtype=torch.int32, device=DEV) for _ in range(3)]
    table = torch.full((2 * 4 * 32,), 77, dtype=torch.int64, device=DEV)
    good = dict(truth=td.data_ptr(), pred=pd.data_ptr(), tlabel=tlabel.data_ptr(), tsize=tsize.data_ptr(), plabel=plabel.data_ptr(),
                psize=psize.data_ptr(), h=5, w=7, K=2, ignore_label=-1, scratch=scratch.data_ptr(), match=m.data_ptr(), inter=inter.data_ptr(),
                cover=cover.data_ptr())
    order_t = ("truth", "tlabel", "tsize", "pred", "plabel", "psize", "match", "inter", "cover", "h", "w", "K", "ignore_label", "table")
    bad = ([{k: None} for k in good if k not in ("h", "w", "K", "ignore_label")] +
           [dict(h=0), dict(w=0), dict(w=-7), dict(h=1 << 16, w=(1 << 14) + 1), dict(K=0), dict(K=33), dict(ignore_label=-2), dict(ignore_label=256)])
    for kw in bad:
        a = dict(good, **kw)
        assert _lib.query("drs_object_match", *[a[k] for k in good], stream()) == 1, kw
        if "scratch" not in kw:
            a["table"] = table.data_ptr()
            assert _lib.query("drs_object_table", *[a[k] for k in order_t], stream()) == 1, kw
    a = dict(good, table=None)
    assert _lib.query("drs_object_table", *[a[k] for k in order_t], stream()) == 1
    torch.cuda.synchronize()
    assert all((t == 77).all() for t in (m, inter, cover, table))
    assert _lib.query("drs_object_scratch_bytes", 0, 7) == 0 == _lib.query("drs_object_scratch_bytes", 1 << 16, (1 << 14) + 1)


# ------------------------------------------------------------------------------------------------------------- 4. validate_test
CH, K6 = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
SIEVE = dict(min_size=(9, 9, 9, 9, 4, 9), connectivity=8)


def _net(seed=5):
    """test_gpu_sieve's net: random moving statistics and a classifier scaled so that the logits have a spread"""
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


def _tiles(d, labels):
    """test_gpu_sieve's pool.  labels "pool": its own labels.  The net is random, so its maps share hardly an object with them;
    labels "near": the net's own plain maps with a seeded 5 % of the pixels moved to another class, and a band of the ignore label 6
    through the first map: many objects found, many missed"""
    from drs_amd import loops
    from drs_amd.synthetic import make_tile
    tiles, labs = zip(*[make_tile(h, w, CH, K6, seed=s, n_seeds=30) for h, w, s in ((44, 50, 21), (37, 61, 22))])
    if labels == "pool":
        return list(tiles), list(labs)
    _, maps = loops.validate_test(d, list(tiles), list(labs), ["a", "b"], 6, MEAN, STD, 25, 7)
    labs = [objects_ref.flipped(m.reshape(lab.shape), K6, frac=0.05, seed=9 + k) for k, (m, lab) in enumerate(zip(maps, labs))]
    labs[0][:, 20:24] = 6
    return list(tiles), labs


@pytest.mark.parametrize("labels, options, c", [("pool", {}, 4), ("near", {}, 4), ("near", dict(sieve=SIEVE), 8)],
                         ids=["pool-plain-4", "near-plain-4", "near-sieve-8"])
def test_validate_test_object_scores(capsys, labels, options, c):
    from drs_amd import loops, metrics as MT
    d = _net()
    tiles, labs = _tiles(d, labels)
    capsys.readouterr()
    res0 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **options)
    text0 = capsys.readouterr().out
    cm1, maps1, extra = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, object_scores=c, **options)
    text1 = capsys.readouterr().out
    ob = extra["objects"]
    assert set(extra) == ({"sieve", "objects"} if options else {"objects"}) and ob["connectivity"] == c
    # the maps, the matrix and every other line are those of the call without the option
    np.testing.assert_array_equal(cm1, res0[0])
    for m0, m1 in zip(res0[1], maps1):
        np.testing.assert_array_equal(m0, m1)
    lines0, lines1 = text0.splitlines(), text1.splitlines()
    mine = [i for i, line in enumerate(lines1) if ": Objects connectivity= %d Truth= [" % c in line]
    assert len(mine) == 3 and mine[-1] == len(lines1) - 1
    assert [line for i, line in enumerate(lines1) if i not in mine] == lines0
    # the tables are the reference's on the maps that were scored (the sieved ones with sieve), ignore label 6
    tables = [objects_ref.table(lab, m.reshape(lab.shape), K6, 6, c) for lab, m in zip(labs, maps1)]
    for k in range(2):
        np.testing.assert_array_equal(ob["per_map"][k]["table"], tables[k])
        if labels == "near":
            assert tables[k][:, 2].sum() > 0 and (tables[k][:, 0].sum(axis=1) > tables[k][:, 2].sum(axis=1)).any()
    np.testing.assert_array_equal(ob["table"], tables[0] + tables[1])
    want = MT.object_scores(tables[0] + tables[1])
    per, whole = objects_ref.scores(tables[0] + tables[1])
    for key in ("precision", "recall", "f1", "sq", "pq"):
        np.testing.assert_array_equal(ob[key], want[key])
        for k in range(K6):
            assert (np.isnan(per[k][key]) and np.isnan(ob[key][k])) or per[k][key] == pytest.approx(ob[key][k], abs=1e-15)
    assert ob["all"]["pq"] == pytest.approx(whole["pq"], abs=1e-15) and (labels == "pool" or 0.0 < ob["all"]["pq"] < 1.0)
    for i, who, o in zip(mine, ("Test Map a: ", "Test Map b: ", "Test ALL MAPS: "), (ob["per_map"][0], ob["per_map"][1], ob)):
        assert lines1[i] == "---- Iter 7 -- " + who + loops._objects_str(c, o)
    # without the option: the same call as ever, the same maps and the same output, and no third value unless another option asks
    res2 = loops.validate_test(d, tiles, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **options)
    assert capsys.readouterr().out == text0 and len(res2) == len(res0) == (3 if options else 2)
    np.testing.assert_array_equal(res2[0], res0[0])
    for m0, m2 in zip(res0[1], res2[1]):
        np.testing.assert_array_equal(m0, m2)
