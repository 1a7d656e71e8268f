"""-m gpu: temperature scaling.  drs_temperature_stats and drs_stitch_finalize_scores_t against the fp64 numpy of
tests/temperature_ref.py, the edges of the definitions, a planted temperature recovered through the kernels, and every inference path
of loops.py with `temperature_beta=`, alone and on two ranks.

Statistics.  Every operation of the kernel is fp64 on the same fp32 inputs as the oracle's, so the two differ by the order of the sums
and a few ulps of exp / log: at most about n x 1.1e-16 < 1e-10 relative at n = 66 049.  The bound is 1e-9: L and H relative to
themselves, G and A relative to A (G cancels; A is its scale).  N is exact.

Score maps (`_check`, the rule of tests/test_gpu_score_maps.py).  With q = 255 s + 0.5 from the oracle (t = float32(beta) v formed in
fp32 as the kernel forms it, the rest fp64), a byte is within 1 of floor(q) everywhere and EQUAL to it wherever q lies farther from
an integer than the band: 1e-3 for sums of logits (pixels inside it at most 0.5 % of a map), 5e-3 for sums of probabilities (at most
2 %), where a 2-ulp logf at |ln q| <= 6.93 times beta = 2.5 moves q by about 1.3e-3; those inputs hold q_k >= 2^-10."""
import os
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402
import temperature_ref as R             # noqa: E402

KINDS = ("confidence", "margin", "entropy")
CH, K6 = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
BAND = {0: (1e-3, 0.005), 1: (5e-3, 0.02)}          # per mode: (band around a rounding tie, largest share of a map inside it)
IGNORE = 6


# ------------------------------------------------------------------------------------------------------------- inputs
def _softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _inputs(n, K, is_prob, seed=0, floor=0.0):
    """sums [n][K] float32, occur in {0, 1, 2, 4} with some zeros, truth bytes 0..8 (6 = ignored; >= K not counted).  Logits:
    4 N(0, 2^2); probabilities: the mean of four softmaxes of such vectors, not below `floor`"""
    rng = np.random.default_rng(7919 * K + 31 * n + 5 * int(is_prob) + seed)
    occur = rng.choice([0, 1, 2, 4], size=n, p=[0.1, 0.3, 0.3, 0.3])
    if n <= 2:
        occur[:] = 2
    if is_prob:
        sums = np.mean([_softmax(rng.normal(size=(n, K)) * 2.0) for _ in range(4)], axis=0)
        sums = np.maximum(sums, floor)
    else:
        sums = 4.0 * rng.normal(size=(n, K)) * 2.0
    truth = rng.integers(0, 9, size=n).astype(np.uint8)
    if n <= 2:
        truth[:] = 1
    return sums.astype(np.float32), occur, truth


_CACHE = {}


def _shared(n, K, is_prob, floor=0.0):
    """one draw per (n, K, mode), shared by the tests that need it and never written to"""
    key = (n, K, is_prob, floor)
    if key not in _CACHE:
        _CACHE[key] = _inputs(n, K, is_prob, floor=floor)
        for a in _CACHE[key]:
            a.setflags(write=False)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------- callers
def _stats(sums, occur, truth, K, is_prob, beta, out=None, ignore=IGNORE):
    """drs_temperature_stats of one map, ADDED to out (a zeroed [5] without one); returns the device tensor"""
    from drs_amd import _lib
    n = int(np.asarray(occur).size)
    s, o, t = dev(np.asarray(sums, dtype=np.float32).reshape(-1)), dev(np.asarray(occur).reshape(-1), torch.int32), dev(np.asarray(truth))
    scratch = torch.full((max(1, _lib.query("drs_temperature_scratch_doubles", n)),), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.zeros(5, dtype=torch.float64, device=DEV) if out is None else out
    _lib.call("drs_temperature_stats", s.data_ptr(), o.data_ptr(), t.data_ptr(), n, K, int(is_prob), ignore, float(beta),
              scratch.data_ptr(), out.data_ptr(), stream())
    torch.cuda.synchronize()
    return out


def _oracle_stats(sums, occur, truth, K, is_prob, beta, ignore=IGNORE):
    return R.stats(R.score_vectors(sums, occur, is_prob), truth, beta, R.counted(occur, truth, K, ignore))


def _assert_stats(got, want, what=""):
    N, L, G, H, A = [float(x) for x in got]
    N0, L0, G0, H0, A0 = want
    print(what, "N %d  dL %.2e  dG/A %.2e  dH %.2e  dA %.2e" % (N0, abs(L - L0) / max(abs(L0), 1e-300), abs(G - G0) / max(A0, 1e-300),
                                                              abs(H - H0) / max(H0, 1e-300), abs(A - A0) / max(A0, 1e-300)))
    assert N == N0
    assert abs(L - L0) <= 1e-9 * abs(L0) and abs(H - H0) <= 1e-9 * abs(H0)
    assert abs(G - G0) <= 1e-9 * A0 and abs(A - A0) <= 1e-9 * A0


def _scores_t(sums, occur, h, w, K, is_prob, beta, want=("labels",) + KINDS, guard=0):
    """drs_stitch_finalize_scores_t into buffers prefilled with 0xAB (`guard` more bytes behind each); a name missing from `want` is
    passed as NULL"""
    from drs_amd import _lib
    s, o = dev(np.asarray(sums, dtype=np.float32).reshape(-1)), dev(np.asarray(occur).reshape(-1), torch.int32)
    bufs = {k: torch.full((h * w + guard,), 0xAB, dtype=torch.uint8, device=DEV) for k in want}
    ptr = [bufs[k].data_ptr() if k in bufs else None for k in ("labels",) + KINDS]
    _lib.call("drs_stitch_finalize_scores_t", s.data_ptr(), o.data_ptr(), h, w, K, int(is_prob), float(beta), ptr[0], ptr[1], ptr[2], ptr[3],
              stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _scores_plain(sums, occur, h, w, K, is_prob):
    from drs_amd import _lib
    s, o = dev(np.asarray(sums, dtype=np.float32).reshape(-1)), dev(np.asarray(occur).reshape(-1), torch.int32)
    bufs = {k: torch.full((h * w,), 0xAB, dtype=torch.uint8, device=DEV) for k in ("labels",) + KINDS}
    _lib.call("drs_stitch_finalize_scores", s.data_ptr(), o.data_ptr(), h, w, K, int(is_prob), *[bufs[k].data_ptr() for k in bufs], stream())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def _finalize(sums, occur, h, w, K):
    from drs_amd import _lib
    s, o = dev(np.asarray(sums, dtype=np.float32).reshape(-1)), dev(np.asarray(occur).reshape(-1), torch.int32)
    out = torch.full((h * w,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.call("drs_stitch_finalize", s.data_ptr(), o.data_ptr(), h, w, K, out.data_ptr(), stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _mismatch(got, q, band):
    """None when the bytes `got` follow the rule of this file's docstring against q, else what breaks it"""
    got = np.asarray(got).reshape(-1).astype(np.int64)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(q)):
        return "oracle not finite"
    want = np.floor(q).astype(np.int64)
    off = np.abs(got - want)
    near = np.abs(q - np.rint(q)) <= band
    print("max |byte - oracle| %d, differing %d, inside the band %d of %d" % (off.max(), (off != 0).sum(), near.sum(), q.size))
    if off.max() > 1:
        return "off by %d" % off.max()
    if (off[~near] != 0).any():
        i = np.flatnonzero((off != 0) & ~near)[0]
        return "%d pixels differ outside the band, first: byte %d, oracle q %.6f" % (((off != 0) & ~near).sum(), got[i], q[i])
    return None


def _check(got, q, is_prob):
    band, cap = BAND[int(bool(is_prob))]
    assert _mismatch(got, q, band) is None, _mismatch(got, q, band)
    q = np.asarray(q).reshape(-1)
    assert (np.abs(q - np.rint(q)) <= band).mean() <= cap


# ------------------------------------------------------------------------------------------------------------- 1. statistics
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257 * 257])
@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_statistics_against_the_fp64_oracle(K, n):
    for is_prob in (0, 1):
        sums, occur, truth = _shared(n, K, is_prob)
        keep = R.counted(occur, truth, K, IGNORE)
        if n > 1000:
            assert 0 < keep.sum() < n and (occur == 0).any() and (truth == IGNORE).any() and (truth >= K).any()
        for beta in (0.25, 1.0, 3.7):
            got = _stats(sums, occur, truth, K, is_prob, beta).cpu().numpy()
            _assert_stats(got, _oracle_stats(sums, occur, truth, K, is_prob, beta), "K %d n %d prob %d beta %g:" % (K, n, is_prob, beta))
        if n > 1000:      # the mutation this exists to catch: the other mode's statistics are not these
            other = _oracle_stats(sums, occur, truth, K, 1 - is_prob, 1.0)
            got = _stats(sums, occur, truth, K, is_prob, 1.0).cpu().numpy()
            assert abs(got[1] - other[1]) > 1e-3 * abs(other[1])


@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_statistics_of_steep_logits_at_the_largest_beta(K):
    """one class at +89, the rest below -60, beta = 64: beta u spans 9 500, far past where exp overflows; with the maximum subtracted
    the winner's p is exactly 1 and H exactly 0"""
    rng = np.random.default_rng(K)
    n = 64 * 5 + 3
    occur = rng.integers(1, 5, size=n)
    v = -rng.uniform(60.0, 89.0, size=(n, K))
    win = rng.integers(0, K, size=n)
    v[np.arange(n), win] = rng.uniform(88.8, 89.0, size=n)
    sums = (occur[:, None] * v).astype(np.float32)
    truth = np.where(rng.uniform(size=n) < 0.5, win, rng.integers(0, K, size=n)).astype(np.uint8)
    got = _stats(sums, occur, truth, K, 0, 64.0, ignore=255).cpu().numpy()          # (no ignored byte: every pixel counts)
    want = _oracle_stats(sums, occur, truth, K, 0, 64.0, ignore=255)
    assert np.all(np.isfinite(got)) and got[0] == n and want[1] > 1e4 and want[3] == 0.0
    _assert_stats(got, want, "steep K %d:" % K)


@pytest.mark.parametrize("K", [2, 6])
def test_statistics_with_a_zero_probability_of_the_true_class(K):
    n = 5000
    sums, occur, truth = [a.copy() for a in _inputs(n, K, 1, seed=9)]
    keep = R.counted(occur, truth, K, IGNORE)
    hit = np.flatnonzero(keep)[::7]
    sums[hit, truth[hit]] = 0.0                                # q_y = 0 on counted pixels: u_y = ln FLT_MIN
    got = _stats(sums, occur, truth, K, 1, 1.0).cpu().numpy()
    want = _oracle_stats(sums, occur, truth, K, 1, 1.0)
    assert np.all(np.isfinite(got)) and want[1] > len(hit) * 80.0          # each such pixel costs about -ln FLT_MIN = 87.3
    _assert_stats(got, want, "q_y = 0, K %d:" % K)


def test_statistics_are_bitwise_reproducible_and_accumulate():
    K = 6
    a = _shared(257 * 257, K, 0)
    b = _shared(257 * 257, K, 1)
    one, again = _stats(*a, K, 0, 0.7), _stats(*a, K, 0, 0.7)
    assert torch.equal(one, again)                              # fixed-order sums: the same bits
    other = _stats(*b, K, 1, 0.7)
    both = _stats(*a, K, 0, 0.7)
    _stats(*b, K, 1, 0.7, out=both)                             # the second map is ADDED in stream order
    assert torch.equal(both, one + other)
    assert float(both[0]) == float(one[0]) + float(other[0]) > 0


def test_statistics_reject_bad_arguments_and_skip_an_empty_map():
    from drs_amd import _lib
    K, n = 6, 100
    sums, occur, truth = _inputs(n, K, 0)
    s, o, t = dev(sums.reshape(-1)), dev(occur, torch.int32), dev(truth)
    scratch = torch.zeros(_lib.query("drs_temperature_scratch_doubles", n), dtype=torch.float64, device=DEV)
    out = torch.zeros(5, dtype=torch.float64, device=DEV)
    ok = [s.data_ptr(), o.data_ptr(), t.data_ptr(), n, K, 0, IGNORE, 1.0, scratch.data_ptr(), out.data_ptr(), stream()]
    assert _lib.query("drs_temperature_stats", *ok) == 0
    for i in (0, 1, 2, 8, 9):                                   # each pointer NULL in turn
        bad = list(ok)
        bad[i] = None
        assert _lib.query("drs_temperature_stats", *bad) == 1
    for i, v in ((4, 0), (4, 9), (3, 1 << 40), (7, 0.0), (7, 1.0 / 65.0), (7, 64.5), (7, -1.0), (7, float("nan")), (7, float("inf"))):
        bad = list(ok)
        bad[i] = v
        assert _lib.query("drs_temperature_stats", *bad) == 1, (i, v)
    torch.cuda.synchronize()
    before = out.clone()
    empty = list(ok)
    empty[3] = 0
    assert _lib.query("drs_temperature_stats", *empty) == 0      # n = 0: nothing is launched, nothing is added
    torch.cuda.synchronize()
    assert torch.equal(out, before) and float(out[0]) > 0
    assert _lib.query("drs_temperature_scratch_doubles", 0) == 0 and _lib.query("drs_temperature_scratch_doubles", 1) == 5
    big = _lib.query("drs_temperature_scratch_doubles", 1 << 39)
    assert big == _lib.query("drs_temperature_scratch_doubles", 1 << 30) and big % 5 == 0      # the grid, and so the rows, are capped


# ------------------------------------------------------------------------------------------------------------- 2. finalising
@pytest.mark.parametrize("is_prob", [0, 1])
@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_beta_one_is_bitwise_the_untempered_entry_point(K, is_prob):
    h = w = 257
    sums, occur, _ = _shared(h * w, K, is_prob, floor=2.0 ** -8 if is_prob else 0.0)
    got, want = _scores_t(sums, occur, h, w, K, is_prob, 1.0), _scores_plain(sums, occur, h, w, K, is_prob)
    for k in ("labels",) + KINDS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_tempered_scores_against_the_oracle_in_both_modes(K):
    h = w = 257
    for is_prob in (0, 1):
        # probabilities: sums >= 2^-8 and occur <= 4, so every q_k >= 2^-10
        sums, occur, _ = _shared(h * w, K, is_prob, floor=2.0 ** -8 if is_prob else 0.0)
        labels = _finalize(sums, occur, h, w, K)
        plain = _scores_plain(sums, occur, h, w, K, is_prob)
        for beta in (0.25, 0.5, 2.5):
            got = _scores_t(sums, occur, h, w, K, is_prob, beta)
            np.testing.assert_array_equal(got["labels"], labels)          # bitwise drs_stitch_finalize's, whatever beta
            lab, q = R.scores_t(sums, occur, is_prob, beta)
            np.testing.assert_array_equal(got["labels"], lab)
            for kind in KINDS:
                _check(got[kind], q[kind], is_prob)
            # the mutations this exists to catch: another beta, or none, does not pass for these bytes
            _, q_other = R.scores_t(sums, occur, is_prob, 1.0 / beta)
            assert _mismatch(got["confidence"], q_other["confidence"], BAND[is_prob][0]) is not None
            assert (got["confidence"] != plain["confidence"]).mean() > 0.05
        cold, hot = _scores_t(sums, occur, h, w, K, is_prob, 2.5), _scores_t(sums, occur, h, w, K, is_prob, 0.25)
        cov = occur > 0
        assert (cold["confidence"][cov].astype(int) >= hot["confidence"][cov].astype(int) - 1).all()      # a larger beta sharpens


@pytest.mark.parametrize("is_prob", [0, 1])
def test_tempered_uncovered_pixels_null_outputs_and_bad_arguments(is_prob):
    from drs_amd import _lib
    K, h, w = 6, 37, 53
    sums, occur, _ = _inputs(h * w, K, is_prob, seed=3, floor=2.0 ** -8 if is_prob else 0.0)
    full = _scores_t(sums, occur, h, w, K, is_prob, 0.5)
    np.testing.assert_array_equal(full["labels"], _finalize(sums, occur, h, w, K))
    unc = occur == 0
    assert unc.any() and (full["confidence"][unc] == 0).all() and (full["margin"][unc] == 0).all() and (full["entropy"][unc] == 255).all()
    assert (full["confidence"][~unc] > 0).all()
    names = ("labels",) + KINDS
    for leave in names:
        part = _scores_t(sums, occur, h, w, K, is_prob, 0.5, want=tuple(n for n in names if n != leave))
        assert leave not in part
        for n in part:
            np.testing.assert_array_equal(part[n], full[n])
    s, o = dev(sums.reshape(-1)), dev(occur, torch.int32)
    lab = torch.zeros(h * w, dtype=torch.uint8, device=DEV)
    call = lambda K_, beta, lab_: _lib.query("drs_stitch_finalize_scores_t", s.data_ptr(), o.data_ptr(), h, w, K_, is_prob, beta, lab_,   # noqa: E731
                                             None, None, None, stream())
    assert call(K, 0.5, lab.data_ptr()) == 0
    assert call(K, 0.5, None) == 1 and call(K, 1.0, None) == 1 and call(9, 0.5, lab.data_ptr()) == 1 and call(9, 1.0, lab.data_ptr()) == 1
    for beta in (0.0, 1.0 / 65.0, 64.5, -2.0, float("nan"), float("inf")):
        assert call(K, beta, lab.data_ptr()) == 1, beta
    assert call(K, 64.0, lab.data_ptr()) == 0 and call(K, 1.0 / 64.0, lab.data_ptr()) == 0
    torch.cuda.synchronize()


def _clear_of_the_band(h, w, K, is_prob, beta):
    """the first draw whose ORACLE puts no score of an h x w map into the band (on a map of 1 to 65 pixels one pixel inside it is over
    the cap): a property of the inputs alone"""
    for seed in range(100, 200):
        sums, occur, _ = _inputs(h * w, K, is_prob, seed=seed, floor=2.0 ** -8 if is_prob else 0.0)
        _, q = R.scores_t(sums, occur, is_prob, beta)
        if all((np.abs(q[k] - np.rint(q[k])) > BAND[is_prob][0]).all() for k in KINDS):
            return sums, occur
    raise AssertionError("no draw clear of the band")


@pytest.mark.parametrize("h, w", [(1, 1), (1, 63), (1, 64), (1, 65), (5, 13), (257, 257)])
def test_tempered_ragged_grid_tails(h, w):
    K, n, beta = 6, h * w, 0.5
    for is_prob in (0, 1):
        if n > 1000:
            sums, occur, _ = _shared(n, K, is_prob, floor=2.0 ** -8 if is_prob else 0.0)
        else:
            sums, occur = _clear_of_the_band(h, w, K, is_prob, beta)
        got = _scores_t(sums, occur, h, w, K, is_prob, beta, guard=64)
        assert all((g[n:] == 0xAB).all() for g in got.values())             # nothing behind the map is written
        lab, q = R.scores_t(sums, occur, is_prob, beta)
        np.testing.assert_array_equal(got["labels"][:n], lab)
        for kind in KINDS:
            _check(got[kind][:n], q[kind], is_prob)


# ------------------------------------------------------------------------------------------------------------- 3. a planted fit
def _ece(sums, occur, truth, h, w, K, is_prob, beta, ignore=IGNORE):
    """ECE of the confidence map at beta, through the kernels: finalise, reliability table, metrics.calibration"""
    from drs_amd import _lib, metrics as MT
    got = _scores_t(sums, occur, h, w, K, is_prob, beta, want=("labels", "confidence"))
    hist = torch.zeros(512, dtype=torch.int64, device=DEV)
    t, p, c = dev(truth), dev(got["labels"]), dev(got["confidence"])
    _lib.call("drs_reliability_histogram", t.data_ptr(), p.data_ptr(), c.data_ptr(), h * w, K, ignore, hist.data_ptr(), stream())
    torch.cuda.synchronize()
    return MT.calibration(hist.cpu().numpy().reshape(256, 2))["ece"]


@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_a_planted_temperature_is_recovered_and_calibrates(K):
    """v ~ N(0, 2^2), the truth drawn from softmax(v), the kernel handed 4 v: a net four times too confident.  The fit finds
    beta = 1/4 and the calibration error of the tempered confidence falls below a quarter of the raw one."""
    from drs_amd import metrics as MT
    h = w = 257
    n = h * w
    rng = np.random.default_rng(40 + K)
    v = rng.normal(size=(n, K)) * 2.0
    truth = (_softmax(v).cumsum(axis=1) < rng.uniform(size=(n, 1))).sum(axis=1).clip(0, K - 1).astype(np.uint8)
    occur = np.ones(n, dtype=np.int64)
    logits = (4.0 * v).astype(np.float32)
    for is_prob, sums in ((0, logits), (1, _softmax(logits.astype(np.float64)).astype(np.float32))):
        # (no ignored byte, 255: every pixel counts, class 6 of K = 8 included)
        fit = MT.fit_temperature(lambda b: _stats(sums, occur, truth, K, is_prob, b, ignore=255).cpu().tolist())
        beta = float(np.float32(fit["beta"]))
        raw, cal = _ece(sums, occur, truth, h, w, K, is_prob, 1.0, 255), _ece(sums, occur, truth, h, w, K, is_prob, beta, 255)
        print("K %d prob %d: beta %.6f, %d evaluations, NLL %.4f -> %.4f, ECE %.4f -> %.4f" % (K, is_prob, beta, fit["iterations"],
                                                                                             fit["nll_before"], fit["nll_after"], raw, cal))
        assert not fit["at_bound"] and not fit["degenerate"] and fit["count"] == n and fit["nll_after"] < fit["nll_before"]
        if not is_prob:
            assert abs(4.0 * beta - 1.0) <= 0.02
        assert cal < 0.25 * raw


# ------------------------------------------------------------------------------------------------------------- 4. every loop path
SPREAD = 16.0


def _net(net_type, b_max, s_max, seed=3, comm=None):
    """a net with random moving statistics and its classifier kernel scaled by SPREAD, as in tests/test_gpu_score_maps.py: the logits
    then have a standard deviation of about 2.4 and the score maps span the byte range"""
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


PATHS = {"windows": (dict(), 0, (101, 109)), "multiscale": (dict(crop_sizes=[25, 18]), 1, (101, 103)),
         "dense": (dict(dense_tile=96), 0, (160, 150)), "dense+flip": (dict(dense_tile=96, dense_tta="flip"), 1, (160, 150))}
PLANTED = 0.5


def _path_sums(d, pool, k, kw, comm=None, bs=6):
    """the accumulators of map k on the path kw names, as that path returns them"""
    from drs_amd import loops
    if "dense_tile" in kw:
        sums, occur, _ = loops.predict_tile_dense(d, pool, k, bs, MEAN, STD, comm, tile=kw["dense_tile"], tta=kw.get("dense_tta"), return_sums=True)
    elif "crop_sizes" in kw:
        sums, occur = loops.predict_tile_multiscale(d, pool, k, kw["crop_sizes"], bs, MEAN, STD, comm, return_sums=True)
    else:
        sums, occur, _ = loops.predict_tile(d, pool, k, 25, bs, MEAN, STD, comm, return_sums=True)
    torch.cuda.synchronize()
    return sums.cpu().numpy().reshape(-1, K6), occur.cpu().numpy().reshape(-1)


def _planted_labels(acc, is_prob, h, w, seed):
    """labels drawn from softmax(PLANTED x u) of the path's own score vectors, a tenth of them the ignored byte: the fit then lies
    inside the bounds, near PLANTED, whatever the random net computes"""
    rng = np.random.default_rng(seed)
    labs = []
    for sums, occur in acc:
        p = _softmax(PLANTED * R.score_vectors(sums, occur, is_prob))
        y = (p.cumsum(axis=1) < rng.uniform(size=(h * w, 1))).sum(axis=1).clip(0, K6 - 1)
        labs.append(np.where(rng.uniform(size=h * w) < 0.1, IGNORE, y).astype(np.uint8).reshape(h, w))
    return labs


def _setup(path, comm=None, bs=6):
    from drs_amd import patches as P
    kw, is_prob, (h, w) = PATHS[path]
    data = [_tile(h, w, seed=21)[0], _tile(h, w, seed=22)[0]]
    d = _net("dilated_grsl", bs, 25, seed=5, comm=comm)
    pool = P.TilePool(data, None, DEV)
    acc = [_path_sums(d, pool, k, kw, comm, bs) for k in range(2)]
    if is_prob and "crop_sizes" in kw:
        assert all((a[1] == len(kw["crop_sizes"])).all() for a in acc)
    return d, data, acc, _planted_labels(acc, is_prob, h, w, seed=2), kw, is_prob, (h, w)


CAL_LINE = re.compile(r"^---- Iter 7 -- Test (Map [ab]|ALL MAPS): Calibration ECE= \d\.\d{6} MCE= \d\.\d{6} Mean Confidence= \d\.\d{6} "
                      r"Accuracy= \d\.\d{6}$")


@pytest.mark.parametrize("path", list(PATHS))
def test_loops_fit_and_apply_a_temperature_on_every_path(path, capsys):
    from drs_amd import loops, metrics as MT
    d, data, acc, labs, kw, is_prob, (h, w) = _setup(path)
    fit = loops.fit_temperature(d, data, labs, 6, MEAN, STD, 25, **kw)
    # the same Newton on the same accumulators, in numpy
    us = np.concatenate([R.score_vectors(s, o, is_prob) for s, o in acc])
    ys = np.concatenate([lb.reshape(-1) for lb in labs])
    keep = np.concatenate([R.counted(o, lb.reshape(-1), K6, IGNORE) for (s, o), lb in zip(acc, labs)])
    want = MT.fit_temperature(lambda b: R.stats(us, ys, b, keep))
    print(path, "beta", fit["beta"], "numpy", want["beta"], "NLL", fit["nll_before"], "->", fit["nll_after"], "pixels", fit["count"])
    assert abs(fit["beta"] - want["beta"]) <= 1e-6 * want["beta"]
    assert fit["nll_after"] <= fit["nll_before"] and fit["count"] == int(keep.sum()) and not fit["at_bound"] and not fit["degenerate"]
    assert abs(fit["beta"] - PLANTED) < 0.05 and fit["beta"] == float(np.float32(fit["beta"]))
    beta = fit["beta"]
    capsys.readouterr()
    cm0, maps0 = loops.validate_test(d, data, labs, ["a", "b"], 6, MEAN, STD, 25, 7, **kw)
    text0 = capsys.readouterr().out
    cm1, maps1, extra1 = loops.validate_test(d, data, labs, ["a", "b"], 6, MEAN, STD, 25, 7, score_maps=KINDS, **kw)
    text1 = capsys.readouterr().out
    cm, maps, extra = loops.validate_test(d, data, labs, ["a", "b"], 6, MEAN, STD, 25, 7, score_maps=KINDS, temperature_beta=beta, **kw)
    text = capsys.readouterr().out
    np.testing.assert_array_equal(cm, cm0)
    for a, b in zip(maps, maps0):
        np.testing.assert_array_equal(a, b)                     # bitwise the labels without the option
    # without a temperature the lines are what they were; with one only the Calibration lines change, by their values and their tail
    ref = lambda t: [ln for ln in t.splitlines() if "Calibration" not in ln]      # noqa: E731
    cal = lambda t: [ln for ln in t.splitlines() if "Calibration" in ln]          # noqa: E731
    assert ref(text) == ref(text1) == text0.splitlines() and "Temperature" not in text1
    assert len(cal(text1)) == 3 and all(CAL_LINE.match(ln) for ln in cal(text1)), cal(text1)
    tail = " Temperature= " + "{:.6f}".format(1.0 / beta)
    assert len(cal(text)) == 3 and all(ln.endswith(tail) and CAL_LINE.match(ln[:-len(tail)]) for ln in cal(text)), cal(text)
    assert extra["temperature_beta"] == beta and "temperature_beta" not in extra1
    # the maps are the oracle's of the path's own accumulators at beta, in the path's mode
    qs = [R.scores_t(s, o, is_prob, beta) for s, o in acc]
    for k in range(2):
        np.testing.assert_array_equal(maps[k].reshape(-1), qs[k][0])
    for kind in KINDS:
        _check(np.concatenate([extra["scores"][k][kind].reshape(-1) for k in range(2)]), np.concatenate([q[1][kind] for q in qs]), is_prob)
    assert (extra["scores"][0]["confidence"] != extra1["scores"][0]["confidence"]).mean() > 0.1
    print(path, "ECE", extra1["calibration"]["ece"], "->", extra["calibration"]["ece"])
    with pytest.raises(ValueError, match="score maps"):
        loops.validate_test(d, data, labs, ["a", "b"], 6, MEAN, STD, 25, 7, temperature_beta=beta, **kw)
    with pytest.raises(ValueError, match="max_resident_bytes"):
        loops.fit_temperature(d, data, labs, 6, MEAN, STD, 25, max_resident_bytes=2 * 4 * (K6 + 1) * h * w - 1, **kw)


def test_generate_final_maps_writes_calibrated_score_files(tmp_path):
    from drs_amd import loops
    h, w = 160, 150
    data = [_tile(h, w, seed=21)[0]]
    labs = [_tile(h, w, seed=21)[1]]
    d = _net("dilated_grsl", 6, 25, seed=5)
    out = str(tmp_path) + "/o_"
    for kw in (dict(), dict(dense_tile=96, dense_tta="flip")):
        maps0, raw = loops.generate_final_maps(d, data, ["7"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", None,
                                               score_maps=("confidence",), **kw)
        maps, scores = loops.generate_final_maps(d, data, ["7"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", out,
                                                 score_maps=("confidence",), temperature_beta=0.5, **kw)
        _, _, extra = loops.validate_test(d, data, labs, ["7"], 6, MEAN, STD, 25, 7, score_maps=("confidence",), temperature_beta=0.5, **kw)
        np.testing.assert_array_equal(maps[0], maps0[0])
        a = np.load(out + "top_mosaic_09cm_area7_class_confidence.npy")
        np.testing.assert_array_equal(a, scores[0]["confidence"])
        np.testing.assert_array_equal(a, extra["scores"][0]["confidence"])          # the same path at the same beta
        assert (a != raw[0]["confidence"]).mean() > 0.1
        with pytest.raises(ValueError, match="score maps"):
            loops.generate_final_maps(d, data, ["7"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", None, temperature_beta=0.5, **kw)


def test_command_line_round_trip(tmp_path, monkeypatch, capsys):
    from drs_amd import cli, loops
    from drs_amd.net import DilatedNet
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path) + "/out_"
    d = DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=4, s_max=25, device=DEV, seed=2)
    loops.save_checkpoint(d, out, 2)
    common = ["isprs_dilated_random.py", "synthetic:70x80x5/vaihingen/", out, out + "model-2"]
    tail = ["a,b", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated_grsl", "single_fixed", "25", "acc"]
    with pytest.raises(SystemExit) as e:
        cli.main(common + tail + ["validate_test", "--score-maps=confidence", "--temperature=auto"], device=DEV)
    assert "temperature_step_2.npy is missing" in str(e.value)
    capsys.readouterr()
    cm, maps, extra = cli.main(common + tail + ["validate_test", "--score-maps=confidence", "--calibrate-temperature"], device=DEV)
    text = capsys.readouterr().out
    saved = np.load(out + "temperature_step_2.npy")
    assert saved.dtype == np.float32 and saved.shape == (1,) and 1.0 / 64.0 <= float(saved[0]) <= 64.0
    beta = float(saved[0])
    assert extra["temperature_beta"] == beta
    line = [ln for ln in text.splitlines() if ln.startswith("---- Iter 2 -- Temperature= ")]
    assert len(line) == 1 and re.match(r"^---- Iter 2 -- Temperature= \d+\.\d{6} Beta= \d+\.\d{6} NLL before= \d+\.\d{6} after= \d+\.\d{6} "
                                       r"Pixels= \d+ Iterations= \d+$", line[0]), line
    assert "Temperature= " + "{:.6f}".format(1.0 / beta) + " Beta= " + "{:.6f}".format(beta) in line[0]
    assert text.index(line[0]) < text.index("Test Map c")                # fitted first, reported after
    assert sum(ln.endswith(" Temperature= " + "{:.6f}".format(1.0 / beta)) for ln in text.splitlines() if "Calibration" in ln) == 2
    cm2, maps2, extra2 = cli.main(["--temperature=auto"] + common + tail + ["validate_test", "--score-maps=confidence"], device=DEV)
    assert extra2["temperature_beta"] == beta
    np.testing.assert_array_equal(extra2["scores"][0]["confidence"], extra["scores"][0]["confidence"])
    np.testing.assert_array_equal(maps2[0], maps[0])
    maps3, scores3 = cli.main(common + tail + ["generate_final_maps", "--score-maps=confidence", "--temperature=auto"], device=DEV)
    np.testing.assert_array_equal(scores3[0]["confidence"], extra["scores"][0]["confidence"])
    np.testing.assert_array_equal(np.load(out + "top_mosaic_09cm_areac_class_confidence.npy"), scores3[0]["confidence"])
    _, _, extra4 = cli.main(common + tail + ["validate_test", "--score-maps=confidence", "--temperature=" + repr(1.0 / beta)], device=DEV)
    np.testing.assert_array_equal(extra4["scores"][0]["confidence"], extra["scores"][0]["confidence"])


# ------------------------------------------------------------------------------------------------------------- 5. two ranks
def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import loops
    from drs_amd.dist import TorchComm
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    res = {}
    for path in ("dense", "dense+flip"):
        d, data, acc, labs, kw, is_prob, _ = _setup(path, comm=comm, bs=1)
        fit = loops.fit_temperature(d, data, labs, 1, MEAN, STD, 25, comm, **kw)
        res[path] = np.array([fit["beta"]], dtype=np.float32)
        res[path + "_count"] = np.array([fit["count"]])
        _, _, extra = loops.validate_test(d, data, labs, ["a", "b"], 1, MEAN, STD, 25, 7, comm=comm, score_maps=("confidence",),
                                          temperature_beta=fit["beta"], **kw)
        res[path + "_confidence"] = extra["scores"][1]["confidence"]
    torch.cuda.synchronize()
    if rank == 1:
        np.savez(out, **res)
    comm.barrier()
    dist.destroy_process_group()


def test_two_ranks_fit_the_same_bits_as_one():
    import tempfile
    from drs_amd import loops
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dp.npz")
        mp.spawn(_dp_worker, args=(2, 31200 + os.getpid() % 1000, out), nprocs=2, join=True)
        r = dict(np.load(out))
    for path in ("dense", "dense+flip"):
        d, data, acc, labs, kw, is_prob, _ = _setup(path, bs=1)
        fit = loops.fit_temperature(d, data, labs, 1, MEAN, STD, 25, **kw)
        # disjoint cores and one tile per forward on both sides, so the ranks' sums add zeros: the accumulators, the labels drawn from
        # them and the fit are bitwise one rank's
        assert r[path].view(np.uint32)[0] == np.array([fit["beta"]], dtype=np.float32).view(np.uint32)[0], (path, r[path], fit["beta"])
        assert int(r[path + "_count"][0]) == fit["count"]
        _, _, extra = loops.validate_test(d, data, labs, ["a", "b"], 1, MEAN, STD, 25, 7, score_maps=("confidence",),
                                          temperature_beta=fit["beta"], **kw)
        np.testing.assert_array_equal(r[path + "_confidence"], extra["scores"][1]["confidence"])
