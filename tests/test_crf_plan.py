"""CPU: the host side of the local dense-CRF refinement: patches.check_crf and the command-line flags, the
temperature-without-scores relaxation, the argument checks of the two entry points (host code: no launch), and properties of the fp64
statement of the rule (tests/crf_ref.py) that the device tests are held to."""
import numpy as np
import pytest

import crf_ref
from drs_amd import patches as P

DEFAULTS = (5, 5, 2, 4.0, 8.0, 0.08, 2.0, 2.0)


# ------------------------------------------------------------------------------------------------------------- check_crf
def test_check_crf_forms():
    assert tuple(P.check_crf(True)) == DEFAULTS and tuple(P.check_crf("crf")) == DEFAULTS
    assert tuple(P.CRF_DEFAULTS) == DEFAULTS == tuple(crf_ref.DEFAULTS[f] for f in P.CrfParams._fields)
    assert tuple(P.check_crf(3)) == (3,) + DEFAULTS[1:]
    assert tuple(P.check_crf(np.int64(10))) == (10,) + DEFAULTS[1:]
    assert tuple(P.check_crf(dict(radius=3, step=4, theta_rgb=0.1))) == (5, 3, 4, 4.0, 8.0, 0.1, 2.0, 2.0)
    assert tuple(P.check_crf({})) == DEFAULTS
    p = P.check_crf((2, 6, 2, 0, 1, 0.5, 0.0, 3))
    assert tuple(p) == (2, 6, 2, 0.0, 1.0, 0.5, 0.0, 3.0) and isinstance(p.w_app, float) and isinstance(p.radius, int)
    assert P.check_crf(list(DEFAULTS)) == P.check_crf(P.check_crf(True)) == P.CRF_DEFAULTS


@pytest.mark.parametrize("bad", [
    None, False, "yes", "", 2.5, (1, 2, 3), DEFAULTS + (1,), dict(radus=3), dict(iters=0), dict(iters=11), 0, 11, -1,
    dict(radius=0), dict(radius=7), dict(step=0), dict(step=5), dict(radius=5, step=3), dict(radius=4, step=4), dict(radius=2.0),
    dict(iters=True), dict(w_app=-1.0), dict(w_smooth=-0.5), dict(theta_xy=0.0), dict(theta_rgb=0), dict(theta_s=-2.0),
    dict(theta_rgb=1e-60), dict(w_app=float("nan")), dict(theta_s=float("inf")), dict(w_smooth="2"), (5, 5, 2, 4.0, 8.0, 0.08, 2.0, None),
])
def test_check_crf_raises_with_the_ranges(bad):
    with pytest.raises(ValueError) as e:
        P.check_crf(bad)
    assert "1..10" in str(e.value) and "radius * step <= 12" in str(e.value) or "unknown parameter" in str(e.value)


def test_check_crf_accepts_the_corners():
    for ok in (dict(radius=6, step=2), dict(radius=3, step=4), dict(radius=4, step=3), dict(radius=1, step=1, iters=1),
               dict(w_app=0.0, w_smooth=0.0), dict(iters=10)):
        P.check_crf(ok)


# ------------------------------------------------------------------------------------------------------------- the command line
ARGV = ["x.py", "a", "b"]


def test_cli_parse_crf_anywhere_in_argv():
    from drs_amd import cli
    got, value = cli.parse_crf(ARGV)
    assert value is None and got == ARGV and got is not ARGV
    assert cli.parse_crf(["--crf"] + ARGV) == (ARGV, P.CRF_DEFAULTS)
    assert cli.parse_crf(ARGV + ["--crf=3"]) == (ARGV, P.CRF_DEFAULTS._replace(iters=3))
    want = P.CrfParams(5, 3, 4, 1.0, 6.0, 0.2, 0.5, 1.5)
    assert cli.parse_crf(["x.py", "--crf-params=3,4,1,6,0.2,0.5,1.5", "a", "b"]) == (ARGV, want)            # alone: implies --crf
    assert cli.parse_crf(["x.py", "a", "--crf-params=3,4,1,6,0.2,0.5,1.5", "b", "--crf=7"]) == (ARGV, want._replace(iters=7))
    for bad, say in ((["--crf=0"], "--crf=ITERS"), (["--crf=11"], "--crf=ITERS"), (["--crf="], "--crf=ITERS"), (["--crf=x"], "--crf=ITERS"),
                     (["--crf", "--crf=2"], "more than once"), (["--crf-params"], "--crf-params="), (["--crf-params=5,2"], "--crf-params="),
                     (["--crf-params=5,3,4,8,0.08,2,2"], "radius * step <= 12"), (["--crf-params=5,2,4,8,0,2,2"], "theta_rgb > 0"),
                     (["--crf-params=5.0,2,4,8,0.08,2,2"], "--crf-params="), (["--crf-params=5,2,4,8,0.08,2, 2"], "--crf-params="),
                     (["--crf-params=5,2,4,8,0.08,2,2"] * 2, "more than once")):
        with pytest.raises(ValueError) as e:
            cli.parse_crf(ARGV + bad)
        assert say in str(e.value), (bad, str(e.value))


MAIN_ARGV = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
             "single_fixed", "25", "acc"]


def test_cli_misuse_exits_as_the_other_flags_do():
    from drs_amd import cli
    from drs_amd.net import NoComm
    for tail, say in ((["training", "--crf"], "--crf applies to the validate_test and generate_final_maps processes only"),
                      (["training", "--crf-params=5,2,4,8,0.08,2,2"], "--crf applies to"),
                      (["validate_test", "--crf=12"], "--crf=ITERS"),
                      (["validate_test", "--crf-params=7,1,4,8,0.08,2,2"], "radius in 1..6"),
                      (["validate_test", "--temperature=2"], "--temperature applies to the score maps only"),
                      (["validate_test", "--crf", "--calibrate-temperature"], "--calibrate-temperature applies to the score maps only")):
        with pytest.raises(SystemExit) as e:
            cli.main(MAIN_ARGV + tail, device="cpu", comm=NoComm())
        assert say in str(e.value), (tail, str(e.value))


class _Reached(Exception):
    pass


@pytest.mark.parametrize("process", ["validate_test", "generate_final_maps"])
@pytest.mark.parametrize("flags, want_crf, want_beta", [
    ([], "absent", None),
    (["--crf"], P.CRF_DEFAULTS, None),
    (["--crf=2", "--temperature=4"], P.CRF_DEFAULTS._replace(iters=2), 0.25),          # a temperature without --score-maps
    (["--crf-params=3,1,1,2,0.1,1,1"], P.CrfParams(5, 3, 1, 1.0, 2.0, 0.1, 1.0, 1.0), None),
])
def test_cli_flags_reach_the_loops(monkeypatch, tmp_path, process, flags, want_crf, want_beta):
    """main parses, loads the synthetic tiles and calls loops.<process>(..., crf=...): the net and the checkpoint are stand-ins, the
    loop itself is intercepted.  Without the flags the loop is called without the argument at all."""
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
    assert seen.get("crf", "absent") == want_crf
    assert seen["temperature_beta"] == want_beta and seen["score_maps"] is None


def test_loops_take_a_temperature_without_scores_only_with_a_crf():
    from drs_amd import loops
    assert loops._check_temperature(0.5, None, P.CRF_DEFAULTS) == 0.5
    assert loops._check_temperature(0.5, ("margin",), P.CRF_DEFAULTS) == 0.5 and loops._check_temperature(None, None, P.CRF_DEFAULTS) is None
    with pytest.raises(ValueError, match="score maps"):
        loops._check_temperature(0.5, None)
    with pytest.raises(ValueError, match="score maps"):
        loops._check_temperature(0.5, None, None)
    with pytest.raises(ValueError, match="1/64"):
        loops._check_temperature(100.0, None, P.CRF_DEFAULTS)
    # the loops refuse before they touch the net: a malformed crf, and a temperature alone
    with pytest.raises(ValueError, match="radius in 1..6"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, crf=dict(radius=9))
    with pytest.raises(ValueError, match="score maps"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, temperature_beta=0.5)
    with pytest.raises(ValueError, match="radius \\* step <= 12"):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, crf=(5, 6, 3, 1, 1, 1, 1, 1))


# ------------------------------------------------------------------------------------------------------------- the entry points' checks
def test_entry_points_reject_bad_arguments_before_any_launch():
    """Argument validation is host code: every rejected call returns DRS_ERR_ARG (raised as DrsError) without touching the device.
    Pointers are dummies; a call that passed validation would launch."""
    from drs_amd import _lib
    _lib.load()
    p, q = 0x1000, 0x2000
    good = dict(q_in=p, logp=p, live=p, tile=p, f64=1, C=5, h=40, w=50, K=6, row0=0, rows=40, R=5, step=2, w_app=4.0, theta_xy=8.0,
                theta_rgb=0.08, w_smooth=2.0, theta_s=2.0, q_out=q)
    bad = [dict(K=1), dict(K=9), dict(C=0), dict(C=9), dict(R=0), dict(R=7), dict(step=0), dict(step=5), dict(R=5, step=3), dict(R=4, step=4),
           dict(w_app=-1.0), dict(w_app=float("nan")), dict(w_smooth=-1.0), dict(w_smooth=float("inf")), dict(theta_xy=0.0),
           dict(theta_rgb=0.0), dict(theta_rgb=-0.08), dict(theta_rgb=1e-30), dict(theta_s=0.0), dict(theta_s=float("nan")),
           dict(row0=-1), dict(rows=0), dict(row0=1), dict(rows=41), dict(h=0), dict(w=0), dict(q_out=p), dict(q_in=None), dict(tile=None),
           dict(logp=None), dict(live=None), dict(q_out=None)]
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(_lib.DrsError, match="DRS_ERR_ARG"):
            _lib.call("drs_crf_step", *[a[k] for k in good], None)
    for args in ((None, p, 4, 4, 6, 0, 1.0, p, p, p), (p, p, 4, 4, 1, 0, 1.0, p, p, p), (p, p, 4, 4, 9, 0, 1.0, p, p, p),
                 (p, p, 0, 4, 6, 0, 1.0, p, p, p), (p, p, 4, 4, 6, 0, 0.0, p, p, p), (p, p, 4, 4, 6, 1, 65.0, p, p, p),
                 (p, p, 4, 4, 6, 0, float("nan"), p, p, p), (p, p, 4, 4, 6, 0, 1.0, p, p, None)):
        with pytest.raises(_lib.DrsError, match="DRS_ERR_ARG"):
            _lib.call("drs_crf_unary", *args, None)


# ------------------------------------------------------------------------------------------------------------- properties of the rule
PARAMS = dict(radius=3, step=2, w_app=4.0, theta_xy=8.0, theta_rgb=0.08, w_smooth=2.0, theta_s=2.0)


@pytest.fixture(scope="module")
def case():
    return crf_ref.synthetic_case(19, 23, 4, 3, seed=5)


def test_ref_without_weights_returns_the_unary(case):
    _, tile, sums, occur = case
    logp, q0, live = crf_ref.unary(sums, occur, False)
    q, _ = crf_ref.refine(sums, occur, False, tile, iters=3, **dict(PARAMS, w_app=0.0, w_smooth=0.0))
    np.testing.assert_allclose(q, q0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(q0.sum(-1), 1.0, atol=1e-12)
    assert not live[-3:, -3:].any() and live.sum() == live.size - 9
    np.testing.assert_allclose(q0[~live], 1.0 / 4, atol=1e-15)              # zero sums: uniform


def test_ref_dead_pixels_never_move_and_never_contribute(case):
    _, tile, sums, occur = case
    q, live = crf_ref.refine(sums, occur, False, tile, iters=3, **PARAMS)
    np.testing.assert_array_equal(q[~live], 0.25)
    # what a dead pixel holds -- its sums, its colour -- reaches nobody: the live pixels' result does not change
    sums2, tile2 = sums.copy(), tile.copy()
    tile2[~live] = 0.123
    q2, _ = crf_ref.refine(sums2, occur, False, tile2, iters=3, **PARAMS)
    np.testing.assert_array_equal(q2[live], q[live])
    # and killing a pixel changes its neighbours exactly as taking it out of their windows does
    occur3 = occur.copy()
    occur3[5, 7] = 0
    q3, _ = crf_ref.refine(sums, occur3, False, tile, iters=1, **PARAMS)
    far = np.ones(live.shape, dtype=bool)
    far[max(0, 5 - 6):5 + 7, max(0, 7 - 6):7 + 7] = False                 # outside the reach R * step = 6 of (5, 7)
    q1, _ = crf_ref.refine(sums, occur, False, tile, iters=1, **PARAMS)
    np.testing.assert_array_equal(q3[far], q1[far])
    assert np.abs(q3[5, 9] - q1[5, 9]).max() > 0                            # (5, 9) = (5, 7) + (0, 1) * step had it as a neighbour


def test_ref_is_invariant_under_a_joint_flip(case):
    _, tile, sums, occur = case
    q, _ = crf_ref.refine(sums, occur, False, tile, iters=2, **PARAMS)
    for flip in (lambda a: a[::-1], lambda a: a[:, ::-1], lambda a: a[::-1, ::-1]):
        qf, _ = crf_ref.refine(flip(sums), flip(occur), False, flip(tile), iters=2, **PARAMS)
        np.testing.assert_allclose(flip(qf), q, rtol=0, atol=1e-13)      # the window is symmetric; only the order of the sum differs


def test_ref_constant_image_appearance_is_a_smoothness_kernel(case):
    _, tile, sums, occur = case
    flat = np.full_like(tile, 0.4)
    a, _ = crf_ref.refine(sums, occur, False, flat, iters=3, **dict(PARAMS, w_app=3.0, theta_xy=2.5, w_smooth=0.0))
    b, _ = crf_ref.refine(sums, occur, False, flat, iters=3, **dict(PARAMS, w_app=0.0, w_smooth=3.0, theta_s=2.5))
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-14)


def test_ref_probability_unary_and_temperature(case):
    _, tile, _, _ = case
    _, _, sums, occur = crf_ref.synthetic_case(19, 23, 4, 3, seed=5, prob=True)
    logp, q0, live = crf_ref.unary(sums, occur, True)
    mean = (sums / np.maximum(occur, 1)[..., None].astype(np.float32)).astype(np.float64)
    mean = mean[live]
    np.testing.assert_allclose(q0[live], mean / mean.sum(-1, keepdims=True), atol=1e-12)      # beta 1: the renormalised mean
    _, qb, _ = crf_ref.unary(sums, occur, True, beta=2.0)
    np.testing.assert_allclose(qb[live], mean ** 2 / (mean ** 2).sum(-1, keepdims=True), atol=1e-12)
    # with a CRF a temperature can change labels: a flat unary lets the image decide
    truth, tile, sums, occur = crf_ref.synthetic_case(24, 24, 4, 3, seed=2)
    weak = dict(iters=2, radius=2, step=1, w_app=1.0, theta_xy=3.0, theta_rgb=0.08, w_smooth=0.0, theta_s=1.0)
    cold, _ = crf_ref.refine(sums, occur, False, tile, beta=8.0, **weak)
    warm, _ = crf_ref.refine(sums, occur, False, tile, beta=1.0 / 16, **weak)
    assert (crf_ref.labels(cold) != crf_ref.labels(warm)).mean() > 0.1
    assert (crf_ref.labels(crf_ref.unary(sums, occur, False, 8.0)[1]) == crf_ref.labels(crf_ref.unary(sums, occur, False, 1 / 16)[1])).all()


def test_ref_cleans_a_noisy_block_map():
    truth, tile, sums, occur = crf_ref.synthetic_case(48, 48, 6, 5, seed=1)
    logp, q0, live = crf_ref.unary(sums, occur, False)
    q, _ = crf_ref.refine(sums, occur, False, tile, **crf_ref.DEFAULTS)
    before = (crf_ref.labels(q0) == truth)[live].mean()
    after = (crf_ref.labels(q) == truth)[live].mean()
    assert before < 0.75 and after > 0.95, (before, after)
