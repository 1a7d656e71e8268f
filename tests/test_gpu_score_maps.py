"""-m gpu: per-pixel score maps.  drs_stitch_finalize_scores and drs_reliability_histogram against fp64 numpy written
here, the edges of the definitions, and every inference path of loops.py with `scores=`: labels unchanged, score maps equal to the
fp64 scores of that path's own accumulators in the mode the path is documented to have, alone and on two ranks.

The comparison rule (`_check`).  A score s is stored as floor(255 s + 0.5) after clamping to [0, 1].  With q = 255 s + 0.5 from the fp64
oracle, the byte must be within 1 of floor(q) everywhere, and EQUAL to it wherever q lies more than 1e-3 from an integer: the
kernel's fp32 arithmetic moves q by well under 1e-4 on these inputs (K <= 8 terms of relative error ~1e-7 on a scale of 255), so
1e-3 leaves an order of magnitude.  The pixels inside that band -- 0.2 % of uniformly spread q, by its width -- may be at most 0.5 %
of a map, so the equality cannot be emptied by the exclusion."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

KINDS = ("confidence", "margin", "entropy")
CH, K6 = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
BAND, CAP = 1e-3, 0.005


# ------------------------------------------------------------------------------------------------------------- the fp64 oracle
def _oracle(sums, occur, is_prob):
    """(labels, {kind: q}) of sums [n][K] (float32 values), occur [n]: fp64 throughout; q = 255 clamp(s) + 0.5, unrounded"""
    sums = np.asarray(sums, dtype=np.float32).astype(np.float64)
    n, K = sums.shape
    occur = np.asarray(occur).reshape(n)
    v = sums / np.where(occur == 0, 1, occur).astype(np.float64)[:, None]
    lab = v.argmax(axis=1)                                       # the first maximum
    if is_prob:
        p = v
    else:
        e = np.exp(v - v.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    rows = np.arange(n)
    conf = p[rows, lab]
    rest = p.copy()
    rest[rows, lab] = -np.inf
    margin = conf - rest.max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    ent = -plogp.sum(axis=1) / np.log(K)
    s = {"confidence": conf, "margin": margin, "entropy": ent}
    unc = occur == 0
    s["confidence"] = np.where(unc, 0.0, s["confidence"])
    s["margin"] = np.where(unc, 0.0, s["margin"])
    s["entropy"] = np.where(unc, 1.0, s["entropy"])
    return lab.astype(np.uint8), {k: 255.0 * np.clip(x, 0.0, 1.0) + 0.5 for k, x in s.items()}


def _mismatch(got, q):
    """None when the bytes `got` follow the rule of this file's docstring against q, else what breaks it"""
    got = np.asarray(got).reshape(-1).astype(np.int64)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(q)):
        return "oracle not finite"
    want = np.floor(q).astype(np.int64)
    off = np.abs(got - want)
    near = np.abs(q - np.rint(q)) <= BAND
    print("max |byte - oracle| %d, differing %d, inside the band %d of %d" % (off.max(), (off != 0).sum(), near.sum(), q.size))
    if off.max() > 1:
        return "off by %d" % off.max()
    if (off[~near] != 0).any():
        i = np.flatnonzero((off != 0) & ~near)[0]
        return "%d pixels differ outside the band, first: byte %d, oracle q %.6f" % (((off != 0) & ~near).sum(), got[i], q[i])
    return None


def _check(got, q):
    assert _mismatch(got, q) is None, _mismatch(got, q)
    q = np.asarray(q).reshape(-1)
    assert (np.abs(q - np.rint(q)) <= BAND).mean() <= CAP


def _finalize(sums, occur, h, w, K):
    from drs_amd import _lib
    s, o = dev(np.asarray(sums, dtype=np.float32).reshape(-1)), dev(np.asarray(occur).reshape(-1), torch.int32)
    out = torch.full((h * w,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.call("drs_stitch_finalize", s.data_ptr(), o.data_ptr(), h, w, K, out.data_ptr(), stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _scores(sums, occur, h, w, K, is_prob, want=("labels",) + KINDS):
    """drs_stitch_finalize_scores into buffers prefilled with 0xAB; a name missing from `want` is passed as NULL"""
    from drs_amd import _lib
    s, o = dev(np.asarray(sums, dtype=np.float32).reshape(-1)), dev(np.asarray(occur).reshape(-1), torch.int32)
    bufs = {k: torch.full((h * w,), 0xAB, dtype=torch.uint8, device=DEV) for k in want}
    ptr = [bufs[k].data_ptr() if k in bufs else None for k in ("labels",) + KINDS]
    _lib.call("drs_stitch_finalize_scores", s.data_ptr(), o.data_ptr(), h, w, K, int(is_prob), ptr[0], ptr[1], ptr[2], ptr[3], stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _case(K, sigma, is_prob, h=37, w=53, seed=0):
    rng = np.random.default_rng(1000 * K + int(10 * sigma) + 7 * int(is_prob) + seed)
    occur = rng.integers(0, 5, size=h * w)
    if is_prob:
        z = rng.normal(size=(h * w, K)) * sigma
        e = np.exp(z - z.max(axis=1, keepdims=True))
        v = e / e.sum(axis=1, keepdims=True)
    else:
        v = rng.normal(size=(h * w, K)) * sigma
    sums = (occur[:, None] * v).astype(np.float32)
    sums[occur == 0] = (rng.normal(size=((occur == 0).sum(), K))).astype(np.float32)      # an uncovered pixel's sums are ignored, but for the label
    return sums, occur


# ------------------------------------------------------------------------------------------------------------- 1. op level
@pytest.mark.parametrize("sigma", [1.0, 2.5])
@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_scores_against_the_fp64_oracle_in_both_modes(K, sigma):
    h, w = 37, 53
    for is_prob in (0, 1):
        sums, occur = _case(K, sigma, is_prob)
        got = _scores(sums, occur, h, w, K, is_prob)
        np.testing.assert_array_equal(got["labels"], _finalize(sums, occur, h, w, K))        # bitwise drs_stitch_finalize's
        lab, q = _oracle(sums, occur, is_prob)
        np.testing.assert_array_equal(got["labels"], lab)
        for kind in KINDS:
            _check(got[kind], q[kind])
        # the mutation this test exists to catch: the other mode's scores do not pass for these bytes
        _, q_swapped = _oracle(sums, occur, 1 - is_prob)
        assert _mismatch(got["confidence"], q_swapped["confidence"]) is not None
        assert _mismatch(got["entropy"], q_swapped["entropy"]) is not None


# ------------------------------------------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_steep_logits_saturate_without_nan(K):
    """|v| up to 89 and a class at -200: exp(88.8) overflows fp32, so a softmax without the max subtraction is inf / inf = NaN here
    (shown below in numpy's fp32); with it the winner has confidence 255, margin 255 and entropy 0"""
    rng = np.random.default_rng(K)
    n = 64 * 5 + 3
    occur = rng.integers(1, 5, size=n)
    v = -rng.uniform(60.0, 89.0, size=(n, K))
    win = rng.integers(0, K, size=n)
    v[np.arange(n), win] = rng.uniform(88.8, 89.0, size=n)
    v[np.arange(n), (win + 1) % K] = -200.0
    sums = (occur[:, None] * v).astype(np.float32)
    got = _scores(sums, occur, 1, n, K, 0)
    np.testing.assert_array_equal(got["labels"], win.astype(np.uint8))
    np.testing.assert_array_equal(got["labels"], _finalize(sums, occur, 1, n, K))
    assert (got["confidence"] == 255).all() and (got["margin"] == 255).all() and (got["entropy"] == 0).all()
    _, q = _oracle(sums, occur, 0)
    for kind in KINDS:
        _check(got[kind], q[kind])
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp((sums / occur[:, None].astype(np.float32)).astype(np.float32))
        assert e.dtype == np.float32 and np.isnan(e / e.sum(axis=1, keepdims=True, dtype=np.float32)).any(axis=1).all()


@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_all_equal_logits(K):
    n = 130
    rng = np.random.default_rng(K)
    occur = rng.integers(1, 5, size=n)
    v = np.repeat(rng.normal(size=(n, 1)) * 3, K, axis=1).astype(np.float32)
    sums = (occur[:, None] * v.astype(np.float64)).astype(np.float32)
    sums = np.repeat(sums[:, :1], K, axis=1)             # exactly equal whatever the rounding did
    got = _scores(sums, occur, 1, n, K, 0)
    assert (got["labels"] == 0).all()                    # the first maximum
    assert (got["confidence"] == int(255.0 / K + 0.5)).all(), got["confidence"][:4]     # 255/K rounded half up: 128, 85, 43, 32
    assert (got["margin"] == 0).all() and (got["entropy"] == 255).all()
    # the same vector given as probabilities
    got = _scores(np.full((n, K), 1.0 / K) * occur[:, None], occur, 1, n, K, 1)
    assert (got["confidence"] == int(255.0 / K + 0.5)).all() and (got["margin"] == 0).all() and (got["entropy"] == 255).all()


@pytest.mark.parametrize("is_prob", [0, 1])
def test_uncovered_pixels_get_the_stated_triple(is_prob):
    K, h, w = 6, 9, 31
    rng = np.random.default_rng(5)
    sums = rng.normal(size=(h * w, K)).astype(np.float32) * 3
    occur = np.zeros(h * w, dtype=np.int64)
    occur[::3] = 2
    got = _scores(sums, occur, h, w, K, is_prob)
    np.testing.assert_array_equal(got["labels"], _finalize(sums, occur, h, w, K))      # the label is as before
    unc = occur == 0
    assert (got["confidence"][unc] == 0).all() and (got["margin"][unc] == 0).all() and (got["entropy"][unc] == 255).all()
    if not is_prob:
        assert (got["confidence"][~unc] > 0).all()


@pytest.mark.parametrize("is_prob", [0, 1])
def test_each_output_may_be_null_and_the_others_do_not_change(is_prob):
    from drs_amd import _lib
    K, h, w = 6, 37, 53
    sums, occur = _case(K, 2.5, is_prob, seed=3)
    full = _scores(sums, occur, h, w, K, is_prob)
    names = ("labels",) + KINDS
    for leave in names:
        part = _scores(sums, occur, h, w, K, is_prob, want=tuple(n for n in names if n != leave))
        assert leave not in part
        for n in part:
            np.testing.assert_array_equal(part[n], full[n])
    only = _scores(sums, occur, h, w, K, is_prob, want=("labels",))
    np.testing.assert_array_equal(only["labels"], full["labels"])
    s, o = dev(sums.reshape(-1)), dev(occur, torch.int32)
    assert _lib.query("drs_stitch_finalize_scores", s.data_ptr(), o.data_ptr(), h, w, K, is_prob, None, None, None, None, stream()) == 1
    lab = torch.zeros(h * w, dtype=torch.uint8, device=DEV)
    assert _lib.query("drs_stitch_finalize_scores", s.data_ptr(), o.data_ptr(), h, w, 9, is_prob, lab.data_ptr(), None, None, None, stream()) == 1


@pytest.mark.parametrize("h, w", [(1, 1), (1, 63), (1, 64), (1, 65), (257, 257)])
def test_ragged_grid_tails(h, w):
    """(on a map of 1 to 65 pixels one pixel inside the band is over the cap, so the draws are the first seed offset, 6, at which the
    ORACLE puts no pixel of the four small maps into the band, in either mode: a property of the inputs alone)"""
    K = 6
    for is_prob in (0, 1):
        sums, occur = _case(K, 2.5, is_prob, h=h, w=w, seed=h * w + 6)
        from drs_amd import _lib
        s, o = dev(sums.reshape(-1)), dev(occur, torch.int32)
        n = h * w
        bufs = [torch.full((n + 64,), 0xAB, dtype=torch.uint8, device=DEV) for _ in range(4)]      # a guard band behind every map
        _lib.call("drs_stitch_finalize_scores", s.data_ptr(), o.data_ptr(), h, w, K, is_prob, *[b.data_ptr() for b in bufs], stream())
        torch.cuda.synchronize()
        got = [b.cpu().numpy() for b in bufs]
        assert all((g[n:] == 0xAB).all() for g in got)
        lab, q = _oracle(sums, occur, is_prob)
        np.testing.assert_array_equal(got[0][:n], lab)
        for g, kind in zip(got[1:], KINDS):
            _check(g[:n], q[kind])


# ------------------------------------------------------------------------------------------------------------- 3. reliability
def _reliability(truth, pred, conf, K, ignore, hist=None):
    from drs_amd import _lib
    hist = torch.zeros(512, dtype=torch.int64, device=DEV) if hist is None else hist
    t, p, c = dev(truth), dev(pred), dev(conf)
    _lib.call("drs_reliability_histogram", t.data_ptr(), p.data_ptr(), c.data_ptr(), truth.size, K, ignore, hist.data_ptr(), stream())
    torch.cuda.synchronize()
    return hist


def _reliability_numpy(truth, pred, conf, K, ignore):
    keep = (truth != ignore) & (truth < K)
    want = np.zeros((256, 2), dtype=np.int64)
    np.add.at(want, (conf[keep].astype(np.int64), 0), 1)
    np.add.at(want, (conf[keep].astype(np.int64), 1), (pred[keep] == truth[keep]).astype(np.int64))
    return want


def test_reliability_histogram_against_numpy():
    rng = np.random.default_rng(11)
    n, K, ignore = 70001, 6, 6
    truth = rng.integers(0, 9, size=n).astype(np.uint8)           # 6 = ignored, 7 and 8 >= K
    pred = np.where(rng.uniform(size=n) < 0.6, np.minimum(truth, K - 1), rng.integers(0, K, size=n)).astype(np.uint8)
    conf = np.minimum(255, rng.gamma(2.0, 40.0, size=n)).astype(np.uint8)
    conf[rng.uniform(size=n) < 0.2] = 255                         # a crowded counter
    want = _reliability_numpy(truth, pred, conf, K, ignore)
    assert want[:, 0].sum() == ((truth < 6)).sum() < n and (want[:, 1] <= want[:, 0]).all() and want[:, 1].sum() > 0
    hist = _reliability(truth, pred, conf, K, ignore)
    np.testing.assert_array_equal(hist.cpu().numpy().reshape(256, 2), want)
    again = _reliability(truth, pred, conf, K, ignore)
    assert torch.equal(hist, again)                               # integer atomics: two runs are bitwise equal
    # the call ADDS: a second map into the same table; another ignore label (none) and another K
    truth2, pred2, conf2 = truth[::-1].copy(), pred[:n].copy(), conf[::-1].copy()
    _reliability(truth2[:5000], pred2[:5000], conf2[:5000], 8, -1, hist)
    want2 = want + _reliability_numpy(truth2[:5000], pred2[:5000], conf2[:5000], 8, -1)
    np.testing.assert_array_equal(hist.cpu().numpy().reshape(256, 2), want2)
    from drs_amd import _lib
    t = dev(truth)
    assert _lib.query("drs_reliability_histogram", t.data_ptr(), t.data_ptr(), t.data_ptr(), n, 9, 6, hist.data_ptr(), stream()) == 1
    assert _lib.query("drs_reliability_histogram", t.data_ptr(), t.data_ptr(), None, n, 6, 6, hist.data_ptr(), stream()) == 1


# ------------------------------------------------------------------------------------------------------------- 4. every loop path
SPREAD = 16.0


def _net(net_type, b_max, s_max, seed=3, comm=None):
    """a net with random moving statistics and its classifier kernel scaled by SPREAD.  The logits of a random-initialised net lie
    within +-0.5 (standard deviation 0.15 on the test tile, by the fp64 oracle): every pixel is then near chance, the entropy map
    spans six bytes and says little about the scoring.  Scaled by 16 the logits have the spread of the op-level cases (standard
    deviation 2.4), the three maps span the byte range and the band of the comparison rule holds its uniform share of about 0.2 %
    of the pixels (by the same oracle) instead of the 0.7 % of the six-byte entropy map."""
    from drs_amd.net import DilatedNet
    rng = np.random.default_rng(seed)
    kw = {} if comm is None else {"comm": comm}
    d = DilatedNet(net_type, CH, K6, 0.005, b_max=b_max, s_max=s_max, device=DEV, seed=seed, **kw)
    for n in d.variable_names():
        v = d.get_variable(n)
        if n.endswith("moving_mean"):
            d.set_variable(n, (rng.normal(size=v.shape) * 0.1).astype(np.float32))
        elif n.endswith("moving_variance"):
            d.set_variable(n, rng.uniform(0.5, 2.0, size=v.shape).astype(np.float32))
    d.set_variable("conv_classifier/weights", d.get_variable("conv_classifier/weights") * np.float32(SPREAD))
    return d


def _tile(h, w, seed):
    from drs_amd.synthetic import make_tile
    return make_tile(h, w, CH, K6, seed=seed, n_seeds=30)


def _check_path(sums, occur, is_prob, labels, smaps, h, w):
    """the maps a path returned against the fp64 scores of its own accumulators in the documented mode -- and not in the other one"""
    sums = sums.cpu().numpy().reshape(h * w, K6)
    occur = occur.cpu().numpy().reshape(h * w)
    lab, q = _oracle(sums, occur, is_prob)
    np.testing.assert_array_equal(labels.cpu().numpy().reshape(-1), lab)
    assert set(smaps) == set(KINDS)
    for kind in KINDS:
        assert smaps[kind].dtype == torch.uint8 and tuple(smaps[kind].shape) == (h, w)
        _check(smaps[kind].cpu().numpy(), q[kind])
    _, q_other = _oracle(sums, occur, not is_prob)
    assert _mismatch(smaps["confidence"].cpu().numpy(), q_other["confidence"]) is not None      # a path wired to the wrong mode fails


DENSE_PATHS = {"plain": (dict(), 0), "flip": (dict(tta="flip"), 1), "d4": (dict(tta="d4"), 1), "scales": (dict(scales=(0.75, 1.25)), 1),
               "scales+flip": (dict(scales=(1.0, 0.75), tta="flip"), 1)}


@pytest.mark.parametrize("path", list(DENSE_PATHS))
def test_dense_paths_keep_their_labels_and_score_their_own_sums(path):
    from drs_amd import loops, patches as P
    kw, is_prob = DENSE_PATHS[path]
    h, w, T_ = 160, 150, 96
    d = _net("dilated_grsl", 1, 24)
    m = max(d.plan.receptive_field)
    assert len(P.dense_axis(h, T_, m, m)[0]) >= 2 and len(P.dense_axis(w, T_, m, m)[0]) >= 2
    pool = P.TilePool([_tile(h, w, seed=12)[0]], None, DEV)
    plain, n0 = loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=T_, **kw)
    pred, n, smaps = loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=T_, scores=KINDS, **kw)
    sums, occur, _ = loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=T_, return_sums=True, **kw)
    torch.cuda.synchronize()
    assert n == n0 and torch.equal(pred, plain)                 # bitwise the labels without the option
    _check_path(sums, occur, is_prob, pred, smaps, h, w)
    only, _, one = loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=T_, scores=("entropy",), **kw)
    assert list(one) == ["entropy"] and torch.equal(one["entropy"], smaps["entropy"]) and torch.equal(only, plain)
    with pytest.raises(ValueError, match="return_sums"):
        loops.predict_tile_dense(d, pool, 0, 2, MEAN, STD, tile=T_, scores=KINDS, return_sums=True, **kw)


def test_window_path_keeps_its_labels_and_scores_its_own_sums():
    from drs_amd import loops, patches as P
    h, w, S, bs = 101, 109, 16, 16          # (11 009 pixels: the band's uniform share of 0.2 % is 22 of them, the cap 55)
    tile, _ = _tile(h, w, seed=4)
    d = _net("dilated_grsl", bs, S)
    assert min(P.window_counts(h, w, S, S // 2)) >= 3
    pool = P.TilePool([tile], None, DEV)
    plain, total0 = loops.predict_tile(d, pool, 0, S, bs, MEAN, STD)
    pred, total, smaps = loops.predict_tile(d, pool, 0, S, bs, MEAN, STD, scores=KINDS)
    sums, occur, _ = loops.predict_tile(d, pool, 0, S, bs, MEAN, STD, return_sums=True)
    torch.cuda.synchronize()
    assert total == total0 and torch.equal(pred, plain)
    assert int(occur.max()) >= 4                                 # overlapping windows: the division matters
    _check_path(sums, occur, 0, pred, smaps, h, w)
    with pytest.raises(ValueError, match="return_sums"):
        loops.predict_tile(d, pool, 0, S, bs, MEAN, STD, scores=KINDS, return_sums=True)


def test_multiscale_window_path_scores_the_mean_of_its_softmax_maps():
    from drs_amd import _lib, loops, patches as P
    h, w, bs, sizes = 101, 103, 16, [25, 18]
    tile, _ = _tile(h, w, seed=8)
    d = _net("dilated_grsl", bs, 25, seed=5)
    pool = P.TilePool([tile], None, DEV)
    plain = loops.predict_tile_multiscale(d, pool, 0, sizes, bs, MEAN, STD)
    pred, smaps = loops.predict_tile_multiscale(d, pool, 0, sizes, bs, MEAN, STD, scores=KINDS)
    # the path's accumulator, as it forms it: the reference's softmax of every size's averaged logits, summed
    acc = torch.zeros(h * w * K6, dtype=torch.float32, device=DEV)
    for s_ in sizes:
        prob, occur, _ = loops.predict_tile(d, pool, 0, s_, bs, MEAN, STD, return_sums=True)
        _lib.call("drs_softmax_accumulate", prob.data_ptr(), occur.data_ptr(), h, w, K6, acc.data_ptr(), d._stream())
    torch.cuda.synchronize()
    assert torch.equal(pred, plain)
    _check_path(acc, torch.full((h * w,), len(sizes), dtype=torch.int32), 1, pred, smaps, h, w)
    assert int(smaps["confidence"].max()) <= 255 and float(smaps["confidence"].float().mean()) < 250      # a mean, not a sum, of the scales


def _reference_lines(text):
    return [ln for ln in text.splitlines() if "Calibration" not in ln]


@pytest.mark.parametrize("path", ["windows", "multiscale", "dense", "dense+d4"])
def test_validate_test_report_and_untouched_reference_lines(path, capsys):
    from drs_amd import loops, metrics as MT
    h, w = (44, 50) if path in ("windows", "multiscale") else (160, 150)
    tiles = [_tile(h, w, seed=21), _tile(h, w, seed=22)]
    data = [t[0] for t in tiles]
    rng = np.random.default_rng(2)
    labs = [np.where(rng.uniform(size=(h, w)) < 0.1, 6, t[1]).astype(np.uint8) for t in tiles]        # 6 = eroded boundary, skipped
    d = _net("dilated_grsl", 6, 25, seed=5)
    kw = {"windows": dict(), "multiscale": dict(crop_sizes=[25, 18]), "dense": dict(dense_tile=96),
          "dense+d4": dict(dense_tile=96, dense_tta="d4")}[path]
    capsys.readouterr()
    cm0, maps0 = loops.validate_test(d, data, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **kw)
    text0 = capsys.readouterr().out
    cm, maps, extra = loops.validate_test(d, data, labs, ["a", "b"], 6, MEAN, STD, 25, 7, score_maps=("entropy",), **kw)
    text = capsys.readouterr().out
    assert text0 == "".join(ln + "\n" for ln in _reference_lines(text)) and "Calibration" not in text0     # character for character
    np.testing.assert_array_equal(cm, cm0)
    for a, b in zip(maps, maps0):
        np.testing.assert_array_equal(a, b)
    cal_lines = [ln for ln in text.splitlines() if "Calibration" in ln]
    assert len(cal_lines) == 3 and cal_lines[0].startswith("---- Iter 7 -- Test Map a: Calibration ECE= ")
    assert cal_lines[2].startswith("---- Iter 7 -- Test ALL MAPS: Calibration ECE= ")
    assert all(" MCE= " in ln and " Mean Confidence= " in ln and " Accuracy= " in ln for ln in cal_lines)
    # "confidence" is added to what was asked for; the table is numpy's of the returned maps
    assert [sorted(s) for s in extra["scores"]] == [["confidence", "entropy"]] * 2
    want = sum(_reliability_numpy(labs[i].reshape(-1), maps[i].reshape(-1), extra["scores"][i]["confidence"].reshape(-1), K6, 6)
               for i in range(2))
    np.testing.assert_array_equal(extra["reliability"], want)
    assert want[:, 0].sum() == sum(int((lb != 6).sum()) for lb in labs) == cm.sum()
    cal = MT.calibration(want)
    assert extra["calibration"]["ece"] == cal["ece"] and extra["calibration"]["accuracy"] == pytest.approx(np.trace(cm) / cm.sum())
    assert len(extra["calibration"]["per_map"]) == 2
    assert "ECE= " + "{:.6f}".format(cal["ece"]) in cal_lines[2]


def test_generate_final_maps_writes_the_score_files(tmp_path):
    from PIL import Image
    from drs_amd import loops
    h, w = 160, 150
    data = [_tile(h, w, seed=21)[0]]
    d = _net("dilated_grsl", 6, 25, seed=5)
    out = str(tmp_path) + "/o_"
    for kw in (dict(), dict(dense_tile=96, dense_tta="flip")):
        maps0 = loops.generate_final_maps(d, data, ["7"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", None, **kw)
        maps, scores = loops.generate_final_maps(d, data, ["7"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", out,
                                                 score_maps=("confidence", "margin"), **kw)
        np.testing.assert_array_equal(maps[0], maps0[0])
        stem = out + "top_mosaic_09cm_area7_class"
        assert os.path.isfile(stem + ".tif") and os.path.isfile(stem + ".npy") and not os.path.exists(stem + "_entropy.npy")
        for kind in ("confidence", "margin"):
            a = np.load(stem + "_" + kind + ".npy")
            assert a.dtype == np.uint8 and a.shape == (h, w)
            np.testing.assert_array_equal(a, scores[0][kind])
            img = Image.open(stem + "_" + kind + ".tif")
            assert img.mode == "L"
            np.testing.assert_array_equal(np.asarray(img), a)
        assert scores[0]["confidence"].std() > 0


def test_command_line_score_maps(tmp_path, monkeypatch, capsys):
    from drs_amd import cli, loops
    from drs_amd.net import DilatedNet
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path) + "/out_"
    d = DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=4, s_max=25, device=DEV, seed=2)
    loops.save_checkpoint(d, out, 2)
    common = ["isprs_dilated_random.py", "synthetic:70x80x5/vaihingen/", out, out + "model-2"]
    tail = ["a,b", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated_grsl", "single_fixed", "25", "acc"]
    cm, maps, extra = cli.main(common + tail + ["validate_test", "--score-maps=margin"], device=DEV)
    assert sorted(extra["scores"][0]) == ["confidence", "margin"] and extra["reliability"][:, 0].sum() == cm.sum()
    assert "Test ALL MAPS: Calibration ECE= " in capsys.readouterr().out
    cm2, maps2, extra2 = cli.main(["--score-maps=confidence"] + common + tail + ["validate_test", "--dense-tile", "--dense-tta=flip"],
                                  device=DEV)
    assert extra2["scores"][0]["confidence"].shape == (70, 80)
    maps3, scores3 = cli.main(common + tail + ["generate_final_maps", "--score-maps=entropy"], device=DEV)
    np.testing.assert_array_equal(maps3[0], maps[0])
    np.testing.assert_array_equal(np.load(out + "top_mosaic_09cm_areac_class_entropy.npy"), scores3[0]["entropy"])
    assert os.path.isfile(out + "top_mosaic_09cm_areac_class_entropy.tif")


# ------------------------------------------------------------------------------------------------------------- 5. two ranks
def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import loops, patches as P
    from drs_amd.dist import TorchComm
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    d = _net("dilated_grsl", 1, 24)
    pool = P.TilePool([_tile(160, 150, seed=12)[0]], None, DEV)
    res = {}
    for name, kw in (("plain", dict()), ("d4", dict(tta="d4"))):
        pred, _, sm = loops.predict_tile_dense(d, pool, 0, 1, MEAN, STD, comm=comm, tile=96, scores=KINDS, **kw)
        res[name + "_labels"] = pred.cpu().numpy()
        for k, v in sm.items():
            res[name + "_" + k] = v.cpu().numpy()
    dw = _net("dilated_grsl", 5, 25, seed=4, comm=comm)
    poolw = P.TilePool([_tile(150, 97, seed=12)[0]], None, DEV)
    pred, total, sm = loops.predict_tile(dw, poolw, 0, 25, 5, MEAN, STD, comm, scores=KINDS)
    res["bands_labels"] = pred.cpu().numpy()
    for k, v in sm.items():
        res["bands_" + k] = v.cpu().numpy()
    torch.cuda.synchronize()
    if rank == 1:                      # any rank holds the whole maps
        np.savez(out, **res)
    comm.barrier()
    dist.destroy_process_group()


def test_two_ranks_gather_the_score_maps(tmp_path):
    from drs_amd import loops, patches as P
    out = str(tmp_path / "dp.npz")
    mp.spawn(_dp_worker, args=(2, 31200 + os.getpid() % 1000, out), nprocs=2, join=True)
    r = np.load(out)
    d = _net("dilated_grsl", 1, 24)
    pool = P.TilePool([_tile(160, 150, seed=12)[0]], None, DEV)
    for name, kw in (("plain", dict()), ("d4", dict(tta="d4"))):
        pred, _, sm = loops.predict_tile_dense(d, pool, 0, 1, MEAN, STD, tile=96, scores=KINDS, **kw)
        np.testing.assert_array_equal(r[name + "_labels"], pred.cpu().numpy())
        for k in KINDS:                # disjoint cores, one tile per forward on both sides: bitwise
            np.testing.assert_array_equal(r[name + "_" + k], sm[k].cpu().numpy(), err_msg=name + " " + k)
    # the window bands: the float sums associate differently where two ranks' bands meet, so within one step of the byte
    dw = _net("dilated_grsl", 5, 25, seed=4)
    poolw = P.TilePool([_tile(150, 97, seed=12)[0]], None, DEV)
    pred, total, sm = loops.predict_tile(dw, poolw, 0, 25, 5, MEAN, STD, scores=KINDS)
    assert P.window_counts(150, 97, 25, 12)[0] >= 2
    assert (r["bands_labels"] != pred.cpu().numpy()).mean() < 1e-3
    for k in KINDS:
        diff = np.abs(r["bands_" + k].astype(np.int64) - sm[k].cpu().numpy().astype(np.int64))
        print(k, "max byte difference", diff.max(), "differing", (diff != 0).mean())
        assert diff.max() <= 1, k
        assert (diff != 0).mean() < 0.01, k
        assert r["bands_" + k].std() > 0
