"""-m gpu: the local dense-CRF refinement (include/drs.h drs_crf_unary / drs_crf_step; loops.refine_crf) against its
fp64 numpy statement tests/crf_ref.py.

Tolerances.  The unary is one op: 1e-5 of the tensor's max, the project's op-level fp32-vs-fp64 standard.  One step fed
the device's own fp32 q_in: 1e-5 absolute (Q <= 1).  Five free-running iterations: 1e-4, the whole-net standard; labels equal wherever
the fp64 top-2 margin exceeds 2e-4 (a Q within 1e-4 cannot swap two classes further apart than that), with at most 0.5 % of the
pixels excluded -- and on these inputs the reference has no live pixel below 1e-3, which the test checks, so the cap hides nothing.
Score bytes (end to end): a score s is stored as floor(255 s + 0.5).  For Q within 1e-4 through logit errors dz <= 1e-4, confidence
moves by <= 1e-4, the margin by <= 2e-4 and the normalised entropy by <= dz (H + 1) / ln K <= 1e-4 (1 + 1 / ln 2) = 2.5e-4: on the 255
scale at most 0.064.  So a byte is within 1 of the reference's everywhere and equal to it wherever 255 s + 0.5 lies more than 0.07
from an integer."""
import numpy as np
import pytest
import torch

import crf_ref

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

PARAMS = dict(w_app=4.0, theta_xy=8.0, theta_rgb=0.08, w_smooth=2.0, theta_s=2.0)
# (h, w, K, C, R, step): ragged against any tile; a map smaller than the window; K at its maximum with dilation; the defaults
SHAPES = [(37, 53, 6, 5, 3, 1), (7, 9, 2, 3, 5, 1), (41, 29, 8, 4, 2, 3), (64, 64, 6, 3, 5, 2)]
IDS = ["37x53-K6-C5-R3-s1", "7x9-K2-C3-R5-s1", "41x29-K8-C4-R2-s3", "64x64-K6-C3-R5-s2"]
_CASES = {}


def _case(shape, prob=False):
    """inputs and the fp64 reference of a shape, computed once and shared by the tests (read-only)"""
    key = (shape, prob)
    if key not in _CASES:
        h, w, K, C, R, s = shape
        truth, tile, sums, occur = crf_ref.synthetic_case(h, w, K, C, seed=0, prob=prob)
        logp, q0, live = crf_ref.unary(sums, occur, prob)
        qs = [q0]
        for _ in range(5):
            qs.append(crf_ref.mean_field_step(qs[-1], logp, live, tile, R, s, **PARAMS))
        for a in (tile, sums, occur, logp, live) + tuple(qs):
            a.setflags(write=False)
        _CASES[key] = dict(tile=tile, sums=sums, occur=occur, logp=logp, live=live, q=qs)
    return _CASES[key]


def _unary(sums, occur, K, prob, beta=1.0):
    from drs_amd import _lib
    h, w = occur.shape
    s, o = dev(np.array(sums).reshape(-1)), dev(occur.astype(np.int32).reshape(-1))          # (copies: the shared inputs are read-only)
    logp = torch.full((h * w * K,), float("nan"), dtype=torch.float32, device=DEV)
    q0 = torch.full_like(logp, float("nan"))
    live = torch.full((h * w,), 7, dtype=torch.int32, device=DEV)
    _lib.call("drs_crf_unary", s.data_ptr(), o.data_ptr(), h, w, K, 1 if prob else 0, beta, logp.data_ptr(), q0.data_ptr(), live.data_ptr(),
              stream())
    return logp, q0, live


def _step(q_in, logp, live, tile_dev, f64, shape, row0=0, rows=None, out=None):
    from drs_amd import _lib
    h, w, K, C, R, s = shape
    out = torch.full_like(q_in, float("nan")) if out is None else out
    _lib.call("drs_crf_step", q_in.data_ptr(), logp.data_ptr(), live.data_ptr(), tile_dev.data_ptr(), 1 if f64 else 0, C, h, w, K, row0,
              h if rows is None else rows, R, s, PARAMS["w_app"], PARAMS["theta_xy"], PARAMS["theta_rgb"], PARAMS["w_smooth"],
              PARAMS["theta_s"], out.data_ptr(), stream())
    return out


def _tile_dev(tile, f64):
    return dev(np.array(tile).reshape(-1), torch.float64 if f64 else torch.float32)


def _ref_tile(tile, f64):
    """what the reference is given: the values as the pool stores them (the kernel reads each as fp32 either way)"""
    return tile if f64 else tile.astype(np.float32)


def _np(t, shape):
    h, w, K = shape[:3]
    return t.cpu().numpy().reshape(h, w, K).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------- 1. the unary
@pytest.mark.parametrize("beta", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("prob", [False, True], ids=["logits", "prob"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_unary(shape, prob, beta):
    h, w, K = shape[:3]
    c = _case(shape, prob)
    logp, q0, live = _unary(c["sums"], c["occur"], K, prob, beta)
    torch.cuda.synchronize()
    want_logp, want_q0, want_live = crf_ref.unary(c["sums"], c["occur"], prob, beta)
    got_logp, got_q0 = _np(logp, shape), _np(q0, shape)
    e_l = np.abs(got_logp - want_logp).max() / np.abs(want_logp).max()
    e_q = np.abs(got_q0 - want_q0).max() / np.abs(want_q0).max()
    print("unary %s prob=%d beta=%g: logp %.2e  q0 %.2e (of the max)" % (shape, prob, beta, e_l, e_q))
    assert e_l <= 1e-5 and e_q <= 1e-5
    np.testing.assert_array_equal(live.cpu().numpy().reshape(h, w), want_live.astype(np.int32))
    assert (~want_live).sum() == min(3, h) * min(3, w)
    np.testing.assert_array_equal(got_q0[~want_live], np.float32(1.0 / K))          # zero sums: exactly uniform


# ------------------------------------------------------------------------------------------------------------- 2. one step
@pytest.mark.parametrize("f64", [True, False], ids=["tile64", "tile32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_teacher_forced_step(shape, f64):
    h, w, K, C, R, s = shape
    c = _case(shape)
    logp, q0, live = _unary(c["sums"], c["occur"], K, False)
    q1 = _step(q0, logp, live, _tile_dev(c["tile"], f64), f64, shape)
    torch.cuda.synchronize()
    want = crf_ref.mean_field_step(_np(q0, shape), c["logp"], c["live"], _ref_tile(c["tile"], f64), R, s, **PARAMS)
    got = _np(q1, shape)
    err = np.abs(got - want).max()
    print("step %s f64=%d: max |dQ| %.2e" % (shape, f64, err))
    assert np.isfinite(got).all() and err <= 1e-5
    np.testing.assert_array_equal(got[~c["live"]], _np(q0, shape)[~c["live"]])       # a dead pixel keeps its Q


# ------------------------------------------------------------------------------------------------------------- 3. five iterations
def _five(shape, f64, prob=False):
    h, w, K, C, R, s = shape
    c = _case(shape, prob)
    logp, qa, live = _unary(c["sums"], c["occur"], K, prob)
    tile = _tile_dev(c["tile"], f64)
    qb = torch.empty_like(qa)
    for _ in range(5):
        _step(qa, logp, live, tile, f64, shape, out=qb)
        qa, qb = qb, qa
    torch.cuda.synchronize()
    return qa, live


@pytest.mark.parametrize("f64", [True, False], ids=["tile64", "tile32"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_five_free_running_iterations(shape, f64):
    from drs_amd import _lib
    h, w, K, C, R, s = shape
    c = _case(shape)
    q, live = _five(shape, f64)
    want = c["q"][5]                      # one reference for both pools: the rule reads every stored value as fp32
    got = _np(q, shape)
    err = np.abs(got - want).max()
    margin = crf_ref.top2_margin(want)
    print("five %s f64=%d: max |dQ| %.2e, smallest live fp64 margin %.2e" % (shape, f64, err, margin[c["live"]].min()))
    assert err <= 1e-4
    assert margin[c["live"]].min() >= 1e-3                   # the reference is decided everywhere: the exclusion below is empty here
    lab = torch.empty(h * w, dtype=torch.uint8, device=DEV)
    _lib.call("drs_stitch_finalize", q.data_ptr(), live.data_ptr(), h, w, K, lab.data_ptr(), stream())
    torch.cuda.synchronize()
    lab = lab.cpu().numpy().reshape(h, w)
    sure = (margin > 2e-4) | ~c["live"]
    assert (~sure).mean() <= 0.005
    np.testing.assert_array_equal(lab[sure], crf_ref.labels(want)[sure])
    np.testing.assert_array_equal(lab[~c["live"]], 0)


def test_five_iterations_from_probabilities():
    shape = SHAPES[0]
    q, _ = _five(shape, True, prob=True)
    err = np.abs(_np(q, shape) - _case(shape, True)["q"][5]).max()
    print("five %s prob: max |dQ| %.2e" % (shape, err))
    assert err <= 1e-4


# ------------------------------------------------------------------------------------------------------------- 4. tiling independence
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_in_bands_and_two_runs_give_the_same_bits(shape):
    h, w, K, C, R, s = shape
    c = _case(shape)
    logp, q0, live = _unary(c["sums"], c["occur"], K, False)
    tile = _tile_dev(c["tile"], True)
    q1 = _step(q0, logp, live, tile, True, shape)
    q_in = _step(q1, logp, live, tile, True, shape)           # a Q that has left the unary: bands read the WHOLE q_in
    whole = _step(q_in, logp, live, tile, True, shape)
    again = _step(q_in, logp, live, tile, True, shape)
    thirds = torch.full_like(q_in, float("nan"))
    cuts = [0, h // 3, 2 * h // 3, h]
    for a, b in zip(cuts[:-1], cuts[1:]):
        _step(q_in, logp, live, tile, True, shape, row0=a, rows=b - a, out=thirds)
    singles = torch.full_like(q_in, float("nan"))
    for y in range(h):
        _step(q_in, logp, live, tile, True, shape, row0=y, rows=1, out=singles)
    torch.cuda.synchronize()
    assert torch.equal(whole, again) and torch.equal(whole, thirds) and torch.equal(whole, singles)
    assert torch.isfinite(whole).all()
    # a band writes its rows and no others
    part = torch.full_like(q_in, float("nan"))
    _step(q_in, logp, live, tile, True, shape, row0=2, rows=3, out=part)
    torch.cuda.synchronize()
    p = part.cpu().numpy().reshape(h, w, K)
    assert np.isnan(p[:2]).all() and np.isnan(p[5:]).all() and np.array_equal(p[2:5], whole.cpu().numpy().reshape(h, w, K)[2:5])


# ------------------------------------------------------------------------------------------------------------- 5. arguments
def test_out_of_range_arguments_return_err_arg_without_a_launch():
    from drs_amd import _lib
    shape = SHAPES[1]
    h, w, K, C, R, s = shape
    c = _case(shape)
    logp, q0, live = _unary(c["sums"], c["occur"], K, False)
    tile = _tile_dev(c["tile"], True)
    out = torch.full_like(q0, float("nan"))
    good = dict(q_in=q0.data_ptr(), logp=logp.data_ptr(), live=live.data_ptr(), tile=tile.data_ptr(), f64=1, C=C, h=h, w=w, K=K, row0=0,
                rows=h, R=R, step=s, q_out=out.data_ptr(), **PARAMS)
    order = ["q_in", "logp", "live", "tile", "f64", "C", "h", "w", "K", "row0", "rows", "R", "step", "w_app", "theta_xy", "theta_rgb",
             "w_smooth", "theta_s", "q_out"]
    bad = [dict(K=1), dict(K=9), dict(C=9), dict(C=0), dict(R=0), dict(R=7), dict(step=0), dict(step=5), dict(R=5, step=3), dict(R=4, step=4),
           dict(w_app=-1.0), dict(w_smooth=-1.0), dict(theta_xy=0.0), dict(theta_rgb=0.0), dict(theta_s=0.0), dict(theta_rgb=float("nan")),
           dict(w_app=float("inf")), dict(row0=-1), dict(rows=0), dict(rows=h + 1), dict(row0=1)]
    for kw in bad:
        a = dict(good, **kw)
        assert _lib.query("drs_crf_step", *[a[k] for k in order], stream()) == 1, kw
    for beta in (0.0, 65.0, float("nan")):
        assert _lib.query("drs_crf_unary", q0.data_ptr(), live.data_ptr(), h, w, K, 0, beta, logp.data_ptr(), out.data_ptr(), live.data_ptr(),
                          stream()) == 1
    for k_bad in (1, 9):
        assert _lib.query("drs_crf_unary", q0.data_ptr(), live.data_ptr(), h, w, k_bad, 0, 1.0, logp.data_ptr(), out.data_ptr(),
                          live.data_ptr(), stream()) == 1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                              # nothing was launched
    assert _lib.query("drs_crf_step", *[good[k] for k in order], stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------------- 6. end to end
CH, K6 = 5, 6
MEAN, STD = np.array([0.5, 0.5, 0.5, 0, 0]), np.array([0.25, 0.25, 0.25, 1, 1])
KINDS = ("confidence", "margin", "entropy")
E2E = {"windows": (dict(), 44, 50), "dense": (dict(dense_tile=96), 160, 150), "dense+flip": (dict(dense_tile=96, dense_tta="flip"), 160, 150)}
CRF = dict(iters=5, radius=5, step=2, **PARAMS)


def _net(seed=5):
    """test_gpu_score_maps' net: random moving statistics and a classifier scaled so that the logits have a spread"""
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


def _check_bytes(got, q, live, what):
    want = crf_ref.score_bytes(q, live)
    K = q.shape[-1]
    lab = np.argmax(q, axis=-1)
    top = np.take_along_axis(q, lab[..., None], axis=-1)[..., 0]
    rest = q.copy()
    np.put_along_axis(rest, lab[..., None], -np.inf, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(q > 0, q * np.log(q), 0.0).sum(axis=-1) / np.log(K)
    s = {"confidence": top, "margin": top - rest.max(axis=-1), "entropy": ent}
    for kind in KINDS:
        g, r = got[kind].astype(np.int64), want[kind].astype(np.int64)
        assert np.abs(g - r).max() <= 1, (what, kind)
        x = 255.0 * np.clip(s[kind], 0.0, 1.0) + 0.5
        clear = (np.abs(x - np.round(x)) > 0.07) | ~live
        assert clear.mean() > 0.75, (what, kind)
        np.testing.assert_array_equal(g[clear], r[clear], err_msg="%s %s" % (what, kind))


@pytest.mark.parametrize("path", list(E2E))
def test_validate_test_and_generate_final_maps_refine_the_paths_sums(path, capsys):
    from drs_amd import loops, patches as P
    kw, h, w = E2E[path]
    from drs_amd.synthetic import make_tile
    tile, lab = make_tile(h, w, CH, K6, seed=21, n_seeds=30)
    d = _net()
    ip = loops.InferencePath(crop_size=25, **kw)
    pool = P.TilePool([tile], [lab], DEV)
    sums, occur, is_prob = ip.run(d, pool, 0, 6, MEAN, STD, loops.NoComm(), return_sums=True)
    assert is_prob == (path == "dense+flip")
    capsys.readouterr()
    cm, maps, extra = loops.validate_test(d, [tile], [lab], ["a"], 6, MEAN, STD, 25, 7, score_maps=KINDS, crf=CRF, **kw)
    text = capsys.readouterr().out
    gmaps, gscores = loops.generate_final_maps(d, [tile], ["a"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", None,
                                               score_maps=KINDS, crf=tuple(CRF[f] for f in P.CrfParams._fields), **kw)
    only = loops.generate_final_maps(d, [tile], ["a"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", None, crf=True, **kw)
    torch.cuda.synchronize()
    q, live = crf_ref.refine(sums.cpu().numpy().reshape(h, w, K6), occur.cpu().numpy().reshape(h, w), is_prob, tile, **CRF)
    assert live.all()
    margin = crf_ref.top2_margin(q)
    sure = margin > 2e-4
    print("e2e %s: %d of %d pixels within 2e-4 of a tie; %.1f %% of the labels moved by the CRF" % (
        path, (~sure).sum(), sure.size, 100.0 * (crf_ref.labels(q) != crf_ref.labels(crf_ref.unary(
            sums.cpu().numpy().reshape(h, w, K6), occur.cpu().numpy().reshape(h, w), is_prob)[1])).mean()))
    assert (~sure).mean() <= 0.005
    for got in (maps[0], gmaps[0], only[0]):
        assert got.dtype == np.uint8 and got.shape == (h, w)
        np.testing.assert_array_equal(got[sure], crf_ref.labels(q)[sure])
    np.testing.assert_array_equal(maps[0], gmaps[0])
    np.testing.assert_array_equal(maps[0], only[0])
    _check_bytes(extra["scores"][0], q, live, path + " validate_test")
    _check_bytes(gscores[0], q, live, path + " generate_final_maps")
    # accuracy, confusion matrix and the printed lines are the refined map's
    want_cm = np.zeros((K6, K6), dtype=np.int64)
    np.add.at(want_cm, (lab[lab != 6], maps[0][lab != 6]), 1)
    np.testing.assert_array_equal(cm, want_cm)
    assert "Overall Accuracy= " + str(int(np.trace(want_cm))) in text and text.count("Calibration ECE=") == 2


def test_crf_none_is_byte_identical_to_not_mentioning_it(capsys):
    from drs_amd import loops
    from drs_amd.synthetic import make_tile
    kw, h, w = E2E["windows"]
    tile, lab = make_tile(h, w, CH, K6, seed=21, n_seeds=30)
    d = _net()
    capsys.readouterr()
    cm0, maps0, ex0 = loops.validate_test(d, [tile], [lab], ["a"], 6, MEAN, STD, 25, 7, score_maps=KINDS)
    text0 = capsys.readouterr().out
    cm1, maps1, ex1 = loops.validate_test(d, [tile], [lab], ["a"], 6, MEAN, STD, 25, 7, score_maps=KINDS, crf=None)
    text1 = capsys.readouterr().out
    assert text0 == text1 and text0
    np.testing.assert_array_equal(cm0, cm1)
    np.testing.assert_array_equal(maps0[0], maps1[0])
    for kind in KINDS:
        np.testing.assert_array_equal(ex0["scores"][0][kind], ex1["scores"][0][kind])
    g0 = loops.generate_final_maps(d, [tile], ["a"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", None)
    g1 = loops.generate_final_maps(d, [tile], ["a"], 6, MEAN, STD, "acc", "single_fixed", [25], "vaihingen", None, crf=None)
    np.testing.assert_array_equal(g0[0], g1[0])
    assert capsys.readouterr().out == ""
    # and with a CRF a temperature is taken without score maps, enters the unary and moves labels
    _, cold = loops.validate_test(d, [tile], [lab], ["a"], 6, MEAN, STD, 25, 7, crf=dict(iters=1, radius=2, step=1, w_app=1.0, w_smooth=0.0),
                                  temperature_beta=8.0)
    _, warm = loops.validate_test(d, [tile], [lab], ["a"], 6, MEAN, STD, 25, 7, crf=dict(iters=1, radius=2, step=1, w_app=1.0, w_smooth=0.0),
                                  temperature_beta=1.0 / 16)
    assert (cold[0] != warm[0]).any()
    with pytest.raises(ValueError, match="score maps"):
        loops.validate_test(d, [tile], [lab], ["a"], 6, MEAN, STD, 25, 7, temperature_beta=0.5)
