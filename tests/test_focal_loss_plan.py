"""Host side of the focal training loss: the fp64 closed form the GPU tests use (tests/focal_ref.py) against torch fp64
autograd, the gamma check, the command-line option, the checkpoint side file.  No GPU: the kernels and the step are held by
tests/test_gpu_focal_loss.py."""
import os

import numpy as np
import pytest
import torch

from drs_amd import cli, loops, patches as P

from focal_ref import focal_closed_form


# ------------------------------------------------------------------------------------------------- the closed form
def _autograd(lg, y, wc, gamma):
    """wc[y] (1 - p_t)^gamma (-log p_t) written with torch ops; per-row terms and the gradient of their sum"""
    t = torch.tensor(lg, dtype=torch.float64, requires_grad=True)
    yy = torch.as_tensor(y, dtype=torch.long)
    logp = torch.log_softmax(t, dim=1).gather(1, yy[:, None])[:, 0]
    pt = torch.exp(logp)
    term = torch.as_tensor(wc, dtype=torch.float64)[yy] * (1.0 - pt) ** gamma * (-logp)
    term.sum().backward()
    return term.detach().numpy(), t.grad.numpy()


def _rows(K, seed):
    """random rows, rows with p_t within 1e-12 of 1 (q in (0, 1e-12], and q == 0 exactly in fp64) and rows with p_t < 1e-6"""
    rng = np.random.default_rng(seed)
    n = 64
    lg = rng.normal(size=(3 * n, K)) * 2.0
    y = rng.integers(0, K, size=3 * n)
    r = np.arange(n, 2 * n)
    lg[r, y[r]] += rng.uniform(29.0, 60.0, size=n) + lg[r].max(axis=1) - lg[r, y[r]]          # the label leads by 29 .. 60: q < K e^-29 < 1e-12
    lg[n:n + 4, :] = 0.0
    lg[np.arange(n, n + 4), y[n:n + 4]] = 800.0                                                 # q == 0 exactly
    r = np.arange(2 * n, 3 * n)
    lg[r, y[r]] -= rng.uniform(15.0, 40.0, size=n) + lg[r, y[r]] - lg[r].min(axis=1)            # the label trails by 15 .. 40: p_t < e^-15 < 1e-6
    return lg, y, n


@pytest.mark.parametrize("K", [2, 3, 6])
@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 5.0])
def test_closed_form_equals_fp64_autograd(gamma, K):
    lg, y, n = _rows(K, seed=10 * K + int(2 * gamma))
    wc = np.asarray([0.5, 2.0, 0.0, 1.25, 7.0, 1.0][:K]) if K != 2 else np.asarray([0.75, 3.5])
    ref = focal_closed_form(lg, y, wc, gamma)
    term, grad = _autograd(lg, y, wc, gamma)
    assert (ref["q"][n:2 * n] <= 1e-12).all() and (ref["q"][n:n + 4] == 0).all() and (ref["q"][n + 4:2 * n] > 0).sum() > 10
    assert (ref["pt"][2 * n:] < 1e-6).all()
    # finite everywhere -- also where autograd is not (gamma < 1 at q == 0: 0^(gamma - 1) * 0)
    assert np.isfinite(ref["term"]).all() and np.isfinite(ref["grad"]).all() and np.isfinite(ref["f"]).all()
    assert (ref["f"][n:n + 4] == 0).all() and (ref["term"][n:n + 4] == 0).all()
    # moderate rows: element by element.  Autograd forms 1 - p_t by subtraction (relative error eps / q) and the closed form does not,
    # so the bound is 1e-9 relative with q > 1e-5 there (random logits of scale 2: q > 1e-5 holds with room, asserted)
    mod = np.r_[0:n, 2 * n:3 * n]
    assert ref["q"][mod].min() > 1e-5
    np.testing.assert_allclose(ref["term"][mod], term[mod], rtol=1e-9, atol=0)
    np.testing.assert_allclose(ref["grad"][mod], grad[mod], rtol=1e-9, atol=1e-9 * np.abs(grad[mod]).max())
    # confident rows: wherever autograd is finite the two agree to 1e-9 of the tensors' maxima (autograd's own 1 - p_t has no correct
    # digit left at q = 1e-12 -- but what it multiplies is below 1e-12 of the maximum)
    fin = np.isfinite(term) & np.isfinite(grad).all(axis=1)
    assert fin[mod].all() and fin[n:2 * n].sum() > 10
    assert np.abs(ref["term"][fin] - term[fin]).max() <= 1e-9 * np.abs(term[fin]).max()
    assert np.abs(ref["grad"][fin] - grad[fin]).max() <= 1e-9 * np.abs(grad[fin]).max()


@pytest.mark.parametrize("K", [2, 3, 6])
def test_gamma_zero_is_the_weighted_cross_entropy(K):
    lg, y, n = _rows(K, seed=K)
    for wc in (np.ones(K), np.linspace(0.0, 3.0, K)):
        ref = focal_closed_form(lg, y, wc, 0.0)
        assert (ref["m"] == 1.0).all() and (ref["f"] == 1.0).all()
        np.testing.assert_array_equal(ref["term"], wc[y] * ref["ce"])
        t = torch.tensor(lg, dtype=torch.float64, requires_grad=True)
        ce = torch.nn.functional.cross_entropy(t, torch.as_tensor(y), reduction="none")
        (torch.as_tensor(wc)[torch.as_tensor(y)] * ce).sum().backward()
        # (torch's log-softmax subtracts numbers of the logits' size, up to 800 here: absolute error eps * 800 = 9e-14 per term, which
        # the closed form's log1p branch does not have)
        np.testing.assert_allclose(ref["term"], (wc[y] * ce.detach().numpy()), rtol=1e-12, atol=wc.max() * 800 * np.finfo(np.float64).eps)
        assert np.abs(ref["grad"] - t.grad.numpy()).max() <= 1e-14 * max(1.0, wc.max())


def test_focal_by_hand():
    # two classes, logits (0, log 3): P = (1/4, 3/4); label 0: q = 3/4, CE = log 4; gamma = 2
    ref = focal_closed_form(np.asarray([[0.0, np.log(3.0)]]), [0], [2.0, 1.0], 2.0)
    m, ce = 0.75 ** 2, np.log(4.0)
    f = m + 2.0 * 0.25 * 0.75 * ce
    np.testing.assert_allclose(ref["term"], [2.0 * m * ce], rtol=1e-14)
    np.testing.assert_allclose(ref["grad"], [[2.0 * f * -0.75, 2.0 * f * 0.75]], rtol=1e-14)


# ------------------------------------------------------------------------------------------------- the gamma check
@pytest.mark.parametrize("bad", [-1.0, -1e-9, float("nan"), float("inf"), -float("inf"), 8.5, 100, "2", None, True, [2.0]])
def test_check_focal_gamma_refuses(bad):
    with pytest.raises(ValueError, match="focal gamma"):
        P.check_focal_gamma(bad)


def test_check_focal_gamma_accepts():
    for g in (0, 0.0, 0.5, 1, 2.0, 5, 8, 8.0, np.float32(0.1), np.int64(3)):
        v = P.check_focal_gamma(g)
        assert isinstance(v, float) and v == float(np.float32(float(g)))         # the float32 the kernels take
    assert P.check_focal_gamma(0.1) == float(np.float32(0.1)) != 0.1
    assert P.parse_focal_gamma("2") == 2.0 and P.parse_focal_gamma("0.5") == 0.5 and P.parse_focal_gamma("0") == 0.0


# ------------------------------------------------------------------------------------------------- command line
def test_cli_good_forms():
    base = ["prog", "a", "b"]
    assert cli.parse_focal_gamma(base) == (base, None)
    assert cli.parse_focal_gamma(base + ["--focal-gamma=2"]) == (base, 2.0)
    assert cli.parse_focal_gamma(["prog", "--focal-gamma=0.5", "a", "b"]) == (base, 0.5)
    assert cli.parse_focal_gamma(["prog", "a", "--focal-gamma=8", "b"]) == (base, 8.0)
    assert cli.parse_focal_gamma(["prog", "a", "--focal-gamma=0", "b"]) == (base, 0.0)
    assert cli.parse_focal_gamma(base + ["--focal-gamma=1e-1"])[1] == float(np.float32(0.1))


@pytest.mark.parametrize("arg", ["--focal-gamma", "--focal-gamma=", "--focal-gamma=-1", "--focal-gamma=nan", "--focal-gamma=inf",
                                 "--focal-gamma=8.5", "--focal-gamma=two", "--focal-gamma=1,2", "--focal-gamma= 2", "--focal-gamma=2 "])
def test_cli_bad_forms_name_the_option_and_the_form(arg):
    with pytest.raises(ValueError) as e:
        cli.parse_focal_gamma(["prog", "a", arg])
    msg = str(e.value)
    assert "--focal-gamma=G" in msg and "(0, 8]" in msg


def test_cli_twice_is_refused():
    with pytest.raises(ValueError, match="--focal-gamma given more than once"):
        cli.parse_focal_gamma(["prog", "--focal-gamma=2", "x", "--focal-gamma=2"])


def test_cli_beside_class_weights_and_the_dense_options():
    """stripped before the positional arguments are counted, in any order with --class-weights and the --dense-* options"""
    argv = ["prog", "--dense-tile=256", "p1", "--focal-gamma=2", "--class-weights=median", "p2", "--dense-tta=d4", "--dense-scales=0.75,1", "p3"]
    argv, tile = cli.parse_dense_tile(argv)
    argv, tta = cli.parse_dense_tta(argv)
    argv, scales = cli.parse_dense_scales(argv)
    argv, se = cli.parse_dense_se(argv)
    argv, cw = cli.parse_class_weights(argv, 6)
    argv, g = cli.parse_focal_gamma(argv)
    assert (argv, tile, tta, scales, se, cw, g) == (["prog", "p1", "p2", "p3"], 256, "d4", (0.75, 1.0), None, "median", 2.0)
    # the other parsers leave the option alone, and it leaves theirs alone
    argv0 = ["prog", "--focal-gamma=2", "x"]
    assert cli.parse_dense_tile(argv0) == (argv0, None) and cli.parse_dense_scales(argv0) == (argv0, None)
    assert cli.parse_class_weights(argv0, 6) == (argv0, None)
    argv1 = ["prog", "--class-weights=1,2", "x"]
    assert cli.parse_focal_gamma(argv1) == (argv1, None)
    # without --class-weights
    assert cli.parse_focal_gamma(cli.parse_class_weights(argv0, 2)[0]) == (["prog", "x"], 2.0)


def test_cli_main_reports_a_bad_option_before_anything_else():
    for main in (cli.main, cli.main_coffee, cli.main_contest):
        with pytest.raises(SystemExit) as e:
            main(["prog", "--focal-gamma=-2"], device="cpu")
        assert "--focal-gamma" in str(e.value) and "(0, 8]" in str(e.value)
        with pytest.raises(SystemExit) as e:
            main(["prog", "--focal-gamma=1", "--focal-gamma=2"], device="cpu")
        assert "--focal-gamma given more than once" in str(e.value)


def test_cli_outside_training_is_refused():
    isprs = ["prog"] + ["x"] * 15
    for process in ("validate_test", "generate_final_maps"):
        with pytest.raises(SystemExit) as e:
            cli.main(isprs + [process, "--focal-gamma=2"], device="cpu")
        assert str(e.value) == "--focal-gamma applies to the training process only"
    contest = ["prog", "--focal-gamma=2"] + ["x"] * 13
    with pytest.raises(SystemExit) as e:
        cli.main_contest(contest + ["test"], device="cpu")
    assert "--focal-gamma applies to the train operation only" in str(e.value)


# ------------------------------------------------------------------------------------------------- checkpoint
class _FakeNet(object):
    """what save_checkpoint / load_checkpoint touch of a net"""

    def __init__(self, K):
        self.K, self._w, self._g = K, None, 0.0
        self.state = {"conv1/weights": np.arange(6, dtype=np.float32), "main_global_step": np.array(0, dtype=np.int64)}

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, d):
        self.state = {k: np.asarray(v) for k, v in d.items()}

    def set_class_weights(self, w):
        self._w = None if w is None else P.check_class_weights(w, self.K)

    @property
    def class_weights(self):
        return None if self._w is None else self._w.copy()

    def set_focal_gamma(self, g):
        self._g = 0.0 if g is None else P.check_focal_gamma(g)

    @property
    def focal_gamma(self):
        return self._g


def test_checkpoint_round_trip_of_gamma(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet(4)
    a.set_focal_gamma(0.1)
    loops.save_checkpoint(a, out, 1000, np.zeros(3, np.float32), np.ones(3, np.int32), np.zeros(3, np.int32))
    assert os.path.isfile(out + "focal_gamma_step_1000.npy") and os.path.isfile(out + "patch_occur_step_1000.npy")
    assert not os.path.exists(out + "class_weights_step_1000.npy")                 # with or without the weights
    side = np.load(out + "focal_gamma_step_1000.npy")
    assert side.dtype == np.float32 and side.shape == () and float(side) == a.focal_gamma
    with np.load(out + "model-1000.npz") as d:
        assert sorted(d.files) == sorted(a.state)            # the model file keeps the TensorFlow variable set: no gamma in it
    b = _FakeNet(4)
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-1000")
    text = capsys.readouterr().out                          # a resumed run says in its log that its loss is focal
    assert "Focal loss (restored from " + out + "focal_gamma_step_1000.npy): gamma 0.1" in text
    assert b.focal_gamma == a.focal_gamma == float(np.float32(0.1))       # the same float32: the same loss
    c = _FakeNet(4)
    loops.load_checkpoint(c, out + "model-1000.npz")
    assert c.focal_gamma == a.focal_gamma
    # beside the class weights
    a.set_class_weights([1, 2, 3, 4])
    loops.save_checkpoint(a, out, 1001)
    assert os.path.isfile(out + "focal_gamma_step_1001.npy") and os.path.isfile(out + "class_weights_step_1001.npy")
    d_ = _FakeNet(4)
    loops.load_checkpoint(d_, out + "model-1001")
    assert d_.focal_gamma == a.focal_gamma and d_.class_weights.tobytes() == a.class_weights.tobytes()


def test_checkpoint_without_gamma_leaves_none(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet(4)
    loops.save_checkpoint(a, out, 7)
    assert not os.path.exists(out + "focal_gamma_step_7.npy")
    a.set_focal_gamma(0)
    loops.save_checkpoint(a, out, 7)
    assert not os.path.exists(out + "focal_gamma_step_7.npy")               # gamma = 0 is unset
    b = _FakeNet(4)
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-7")
    assert b.focal_gamma == 0.0 and "Focal loss" not in capsys.readouterr().out
    # a checkpoint of another step's gamma is not picked up
    a.set_focal_gamma(2)
    loops.save_checkpoint(a, out, 8)
    loops.load_checkpoint(b, out + "model-7")
    assert b.focal_gamma == 0.0


def test_setup_focal_gamma_overrides_and_says_so(capsys):
    from drs_amd.net import NoComm
    lines = []
    net = _FakeNet(4)
    assert loops.setup_focal_gamma(net, 0, NoComm(), lines.append) == 0.0 and lines == [] and net.focal_gamma == 0.0
    assert loops.setup_focal_gamma(net, 2, NoComm(), lines.append) == 2.0 and net.focal_gamma == 2.0
    assert len(lines) == 1 and "Focal loss: gamma 2" in lines[0] and "replacing" not in lines[0]
    loops.setup_focal_gamma(net, 0.5, NoComm(), lines.append)
    assert len(lines) == 2 and "gamma 0.5" in lines[1] and "replacing the gamma restored from the checkpoint, 2" in lines[1]
    loops.setup_focal_gamma(net, 0, NoComm(), lines.append)
    assert net.focal_gamma == 0.0 and len(lines) == 3 and "gamma 0" in lines[2] and "replacing" in lines[2]
    with pytest.raises(ValueError):
        loops.setup_focal_gamma(net, 9, NoComm(), lines.append)
