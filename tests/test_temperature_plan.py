"""CPU: the host side of temperature scaling: metrics.fit_temperature on statistics computed in numpy
(tests/temperature_ref.py), against a derivative-free minimiser, under a rescaling of the accumulators, at both bounds and on
degenerate data; and the command-line options with their misuse errors."""
import numpy as np
import pytest

from drs_amd import metrics as MT
from drs_amd import patches as P
from temperature_ref import golden_section, stats

N_PIX, SIGMA = 257 * 257, 8.0


def _data(K, seed=0, sigma=SIGMA, n=N_PIX):
    """n pixels of logits u ~ N(0, sigma^2) with the truth drawn from softmax(u / 3): the fit's beta is near 1/3, away from 1 and
    from both bounds"""
    rng = np.random.default_rng(100 * K + seed)
    u = rng.normal(size=(n, K)) * sigma
    t = u / 3.0
    p = np.exp(t - t.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    y = (p.cumsum(axis=1) < rng.uniform(size=(n, 1))).sum(axis=1).clip(0, K - 1)
    return u, y


def _counting(u, y):
    calls = []

    def fn(beta):
        calls.append(beta)
        return stats(u, y, beta)
    return fn, calls


@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_fit_reaches_the_stationary_point_and_agrees_with_golden_section(K):
    u, y = _data(K)
    fn, calls = _counting(u, y)
    fit = MT.fit_temperature(fn)
    _, L, G, H, A = stats(u, y, fit["beta"])
    print("K", K, "beta", fit["beta"], "|G|/A", abs(G) / A, "evaluations", len(calls))
    assert abs(G) <= 1e-10 * A
    assert not fit["at_bound"] and not fit["degenerate"] and fit["count"] == N_PIX
    assert fit["iterations"] == len(calls) <= 2 + 60
    assert calls[0] == 1.0 / 64.0 and calls[1] == 64.0 and calls[2] == 1.0          # the two ends, then the start
    assert fit["temperature"] == pytest.approx(1.0 / fit["beta"], rel=1e-15)
    assert fit["nll_before"] == pytest.approx(stats(u, y, 1.0)[1] / N_PIX, rel=1e-15)
    assert fit["nll_after"] == pytest.approx(L / N_PIX, rel=1e-15) and fit["nll_after"] < fit["nll_before"]
    assert abs(fit["beta"] - 1.0 / 3.0) < 0.02                                     # the planted value
    gold = golden_section(u, y)
    # golden section locates the minimum of a smooth L only to about sqrt(eps): a shift d in ln beta changes L by H beta^2 d^2 / 2,
    # invisible once below eps L, i.e. d ~ sqrt(2 eps L / (H beta^2)) ~ 1e-8 here; 1e-6 leaves two orders
    assert abs(fit["beta"] - gold) <= 1e-6 * gold, (fit["beta"], gold)


@pytest.mark.parametrize("K", [2, 3, 6, 8])
def test_accumulators_times_four_give_a_quarter_of_beta(K):
    """multiplying every score by 4 (exact in binary floating point) maps L(beta) onto L(beta / 4)"""
    u, y = _data(K, seed=1)
    one = MT.fit_temperature(lambda b: stats(u, y, b))["beta"]
    four = MT.fit_temperature(lambda b: stats(4.0 * u, y, b))["beta"]
    print("K", K, "ratio error", abs(4.0 * four / one - 1.0))
    assert abs(4.0 * four / one - 1.0) <= 1e-9


@pytest.mark.parametrize("K", [2, 6])
def test_separable_data_ends_at_the_upper_bound_and_all_wrong_at_the_lower(K):
    u, _ = _data(K, seed=2, n=4001)
    right = u.argmax(axis=1)
    fn, calls = _counting(u, right)
    fit = MT.fit_temperature(fn)
    assert fit["beta"] == 64.0 and fit["at_bound"] and not fit["degenerate"] and len(calls) <= 3
    assert fit["nll_after"] < fit["nll_before"] == pytest.approx(stats(u, right, 1.0)[1] / 4001, rel=1e-15)
    wrong = u.argmin(axis=1)
    fit = MT.fit_temperature(lambda b: stats(u, wrong, b))
    assert fit["beta"] == 1.0 / 64.0 and fit["at_bound"] and fit["temperature"] == 64.0
    assert fit["nll_after"] < fit["nll_before"]
    # other bounds are taken as given
    fit = MT.fit_temperature(lambda b: stats(u, right, b), lo=0.5, hi=2.0)
    assert fit["beta"] == 2.0 and fit["at_bound"]


def test_no_pixels_and_one_class_are_degenerate():
    fit = MT.fit_temperature(lambda b: (0.0, 0.0, 0.0, 0.0, 0.0))
    assert fit["beta"] == 1.0 and fit["temperature"] == 1.0 and fit["degenerate"] and not fit["at_bound"] and fit["count"] == 0
    assert fit["nll_before"] == 0.0 and fit["nll_after"] == 0.0
    u = np.random.default_rng(0).normal(size=(50, 1))
    fit = MT.fit_temperature(lambda b: stats(u, np.zeros(50, dtype=np.int64), b))
    assert fit["beta"] == 1.0 and fit["degenerate"] and fit["count"] == 50 and fit["nll_before"] == 0.0 == fit["nll_after"]


def test_fit_honours_max_iter_and_rejects_bad_bounds():
    u, y = _data(3, seed=3, n=5000)
    fn, calls = _counting(u, y)
    fit = MT.fit_temperature(fn, max_iter=2)
    assert len(calls) == 4 == fit["iterations"] and fit["beta"] == calls[-1]
    for kw in (dict(lo=0.0), dict(lo=2.0), dict(hi=0.5), dict(hi=float("inf")), dict(lo=float("nan")), dict(max_iter=0)):
        with pytest.raises(ValueError):
            MT.fit_temperature(fn, **kw)


def test_bisection_takes_over_where_newton_leaves_the_bracket():
    """a curvature reported far too small throws every Newton proposal out of the bracket: the geometric mean still converges"""
    u, y = _data(3, seed=4, n=5000)

    def flat(beta):
        N, L, G, H, A = stats(u, y, beta)
        return N, L, G, H * 1e-6, A
    fit = MT.fit_temperature(flat, max_iter=60)
    want = MT.fit_temperature(lambda b: stats(u, y, b))["beta"]
    assert abs(fit["beta"] - want) <= 1e-9 * want and fit["iterations"] <= 62
    fit = MT.fit_temperature(lambda b: stats(u, y, b)[:3] + (0.0,) + stats(u, y, b)[4:])          # H <= 0: the same
    assert abs(fit["beta"] - want) <= 1e-9 * want


# ------------------------------------------------------------------------------------------------------------- the option values
def test_check_temperature_beta():
    assert P.BETA_MIN == 1.0 / 64.0 and P.BETA_MAX == 64.0
    assert P.check_temperature_beta(1) == 1.0 and P.check_temperature_beta(64.0) == 64.0 and P.check_temperature_beta(1.0 / 64.0) == 1.0 / 64.0
    assert P.check_temperature_beta(0.3) == float(np.float32(0.3))             # the float32 the kernel takes
    for bad in (0.0, -1.0, 64.5, 0.01, float("nan"), float("inf"), "1", None, True, [1.0]):
        with pytest.raises(ValueError, match="1/64"):
            P.check_temperature_beta(bad)


@pytest.mark.parametrize("text, want", [("auto", "auto"), ("1", 1.0), ("2", 0.5), ("0.25", 4.0), ("64", 1.0 / 64.0), ("1.5", float(np.float32(1 / 1.5)))])
def test_parse_temperature_accepts(text, want):
    assert P.parse_temperature(text) == want


@pytest.mark.parametrize("text", ["", "0", "-2", "nan", "inf", " 2", "2 ", "Auto", "warm", "65", "0.01", "1,2"])
def test_parse_temperature_rejects(text):
    with pytest.raises(ValueError) as e:
        P.parse_temperature(text)
    assert "auto" in str(e.value) and repr(text) in str(e.value)


# ------------------------------------------------------------------------------------------------------------- the command line
def test_cli_parsers_anywhere_in_argv():
    from drs_amd import cli
    argv = ["x.py", "a", "b"]
    assert cli.parse_temperature(argv) == (argv, None) and cli.parse_calibrate_temperature(argv) == (argv, None)
    assert cli.parse_temperature(["--temperature=auto"] + argv) == (argv, "auto")
    assert cli.parse_temperature(argv + ["--temperature=4"]) == (argv, 0.25)
    assert cli.parse_calibrate_temperature(["x.py", "--calibrate-temperature", "a", "b"]) == (argv, True)
    for bad, say in ((["--temperature"], "--temperature=auto"), (["--temperature="], "--temperature=auto"),
                     (["--temperature=0"], "T > 0"), (["--temperature=cold"], "--temperature=auto"),
                     (["--temperature=2", "--temperature=auto"], "more than once")):
        with pytest.raises(ValueError) as e:
            cli.parse_temperature(argv + bad)
        assert say in str(e.value)
    for bad, say in ((["--calibrate-temperature=1"], "takes no value"), (["--calibrate-temperature"] * 2, "more than once")):
        with pytest.raises(ValueError) as e:
            cli.parse_calibrate_temperature(argv + bad)
        assert say in str(e.value)
    assert cli.temperature_file("out_", 7) == "out_temperature_step_7.npy"


def test_cli_misuse_exits_as_the_other_flags_do():
    from drs_amd import cli
    from drs_amd.net import NoComm
    argv = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
            "single_fixed", "25", "acc"]
    sm = "--score-maps=confidence"
    for tail, say in ((["validate_test", "--calibrate-temperature"], "--calibrate-temperature applies to the score maps only"),
                      (["validate_test", "--temperature=2"], "--temperature applies to the score maps only"),
                      (["generate_final_maps", sm, "--calibrate-temperature"], "--calibrate-temperature applies to the validate_test process only"),
                      (["training", sm, "--calibrate-temperature"], "applies"),
                      (["training", "--temperature=auto"], "applies"),
                      (["validate_test", sm, "--calibrate-temperature", "--temperature=2"], "cannot be given as well"),
                      (["validate_test", sm, "--temperature=0"], "--temperature=auto"),
                      (["validate_test", sm, "--temperature=2", "--temperature=2"], "more than once"),
                      (["validate_test", sm, "--calibrate-temperature=yes"], "takes no value")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv + tail, device="cpu", comm=NoComm())
        assert say in str(e.value), (tail, str(e.value))


def test_loops_need_scores_for_a_temperature():
    from drs_amd import loops
    assert loops._check_temperature(None, None) is None and loops._check_temperature(None, ("margin",)) is None
    assert loops._check_temperature(0.5, ("margin",)) == 0.5
    with pytest.raises(ValueError, match="score maps"):
        loops._check_temperature(0.5, None)
    with pytest.raises(ValueError, match="1/64"):
        loops._check_temperature(100.0, ("margin",))
