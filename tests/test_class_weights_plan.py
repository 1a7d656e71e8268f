"""Host side of the class-weighted training loss: the weight recipes, the command-line option, the checkpoint side file.
No GPU: the kernels and the step are held by tests/test_gpu_class_weights.py."""
import math
import os

import numpy as np
import pytest

from drs_amd import cli, loops, patches as P


# ------------------------------------------------------------------------------------------------- recipes
def test_balanced_by_hand():
    # N = 100, three classes occur: wc_k = 100 / (3 n_k)
    w = P.class_weights([50, 30, 20], "balanced")
    assert w.dtype == np.float64
    np.testing.assert_allclose(w, [100 / 150.0, 100 / 90.0, 100 / 60.0], rtol=1e-15)


def test_balanced_with_a_class_that_never_occurs():
    # class 2 has no pixel: Kp = 3, N = 1000, its weight is 1
    w = P.class_weights([600, 390, 0, 10], "balanced")
    np.testing.assert_allclose(w, [1000 / 1800.0, 1000 / 1170.0, 1.0, 1000 / 30.0], rtol=1e-15)


def test_median_by_hand():
    # f = (.5, .3, .2): median .3
    w = P.class_weights([50, 30, 20], "median")
    np.testing.assert_allclose(w, [0.6, 1.0, 1.5], rtol=1e-15)
    # four occurring classes and an absent one: the median runs over the occurring ones, (0.2 + 0.3) / 2
    w = P.class_weights([10, 20, 0, 30, 40], "median")
    np.testing.assert_allclose(w, [2.5, 1.25, 1.0, 0.25 / 0.3, 0.625], rtol=1e-15)


def test_counts_with_a_void_label_left_out():
    """the contest flavour: label 7 is void and is not counted (what TilePool.label_counts does on the device, in numpy here)"""
    rng = np.random.default_rng(0)
    lab = rng.choice(8, size=(40, 50), p=[0.3, 0.2, 0.2, 0.1, 0.05, 0.03, 0.02, 0.1]).astype(np.uint8)
    counts = np.bincount(lab[lab != 7].reshape(-1), minlength=7)[:7]
    w = P.class_weights(counts, "balanced")
    N = int((lab != 7).sum())
    np.testing.assert_allclose(w, N / (7.0 * counts), rtol=1e-15)
    assert abs(float(np.sum(counts / N * w)) - 1.0) < 1e-12


@pytest.mark.parametrize("counts", [[50, 30, 20], [600, 390, 0, 10], [1, 10 ** 9, 12345, 0, 7, 99999, 3, 2 ** 40], [5]])
def test_balanced_keeps_the_scale_of_the_loss(counts):
    """sum_k f_k wc_k = 1: with the pixel-count normaliser the expected weighted loss has the scale of the unweighted one"""
    n = np.asarray(counts, dtype=np.int64)
    w = P.class_weights(n, "balanced")
    f = n / float(n.sum())
    assert abs(float(np.sum(f * w)) - 1.0) < 1e-12
    assert np.all(w[n == 0] == 1.0)


def test_no_pixels_at_all_gives_ones():
    np.testing.assert_array_equal(P.class_weights([0, 0, 0], "balanced"), [1, 1, 1])
    np.testing.assert_array_equal(P.class_weights([0, 0, 0], "median"), [1, 1, 1])


def test_explicit_list_round_trips():
    given = [0.5, 2.0, 0.0, 1.25, 3.0, 1.0]
    w = P.class_weights([1, 2, 3, 4, 5, 6], given)
    np.testing.assert_array_equal(w, given)
    w32 = P.check_class_weights(list(w), 6)
    assert w32.dtype == np.float32 and w32.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(w32, np.asarray(given, dtype=np.float32))
    np.testing.assert_array_equal(P.check_class_weights(tuple(given), 6), w32)
    np.testing.assert_array_equal(P.check_class_weights(w32, 6), w32)


@pytest.mark.parametrize("bad,K", [([1.0, 2.0], 3), ([1.0, -0.5, 1.0], 3), ([1.0, float("nan"), 1.0], 3), ([1.0, float("inf"), 1.0], 3),
                                   ([1.0, 1e39, 1.0], 3), ("balanced", 3), ([1.0] * 9, 9), (None, 3), (["a", 1.0, 2.0], 3), ([True, 1.0, 2.0], 3)])
def test_bad_weights_are_refused(bad, K):
    with pytest.raises(ValueError):
        P.check_class_weights(bad, K)


def test_bad_recipes_and_counts_are_refused():
    with pytest.raises(ValueError):
        P.class_weights([1, 2, 3], "inverse")
    with pytest.raises(ValueError):
        P.class_weights([1, 2, 3], [1.0, 2.0])
    with pytest.raises(ValueError):
        P.class_weights([1, -2, 3], "balanced")
    with pytest.raises(ValueError):
        P.class_weights([1.5, 2.0], "balanced")
    with pytest.raises(ValueError):
        P.class_weights([1] * 9, "balanced")


# ------------------------------------------------------------------------------------------------- command line
def test_cli_good_forms():
    base = ["prog", "a", "b"]
    assert cli.parse_class_weights(base) == (base, None)
    assert cli.parse_class_weights(base + ["--class-weights=balanced"]) == (base, "balanced")
    assert cli.parse_class_weights(["prog", "--class-weights=median", "a", "b"], 6) == (base, "median")
    rest, cw = cli.parse_class_weights(["prog", "a", "--class-weights=1,2.5,0,1e-1,3,1", "b"], 6)
    assert rest == base and cw == (1.0, 2.5, 0.0, 0.1, 3.0, 1.0)
    assert cli.parse_class_weights(base + ["--class-weights=0.25,4"], 2)[1] == (0.25, 4.0)
    assert cli.parse_class_weights(base + ["--class-weights=0.25,4"])[1] == (0.25, 4.0)       # count checked where the net is known


@pytest.mark.parametrize("arg,K", [("--class-weights", 6), ("--class-weights=", 6), ("--class-weights=1,2,3", 6), ("--class-weights=1,2,3,4,5,6,7", 6),
                                   ("--class-weights=1,-2", 2), ("--class-weights=1,nan", 2), ("--class-weights=inf,1", 2),
                                   ("--class-weights=1,,2", 2), ("--class-weights=1, 2", 2), ("--class-weights=inverse", 2),
                                   ("--class-weights=1,2,3,4,5,6,7,8,9", None)])
def test_cli_bad_forms_name_the_option_and_the_form(arg, K):
    with pytest.raises(ValueError) as e:
        cli.parse_class_weights(["prog", "a", arg], K)
    msg = str(e.value)
    assert "--class-weights" in msg and "balanced|median|w0,w1,..." in msg


def test_cli_twice_is_refused():
    with pytest.raises(ValueError, match="more than once"):
        cli.parse_class_weights(["prog", "--class-weights=balanced", "--class-weights=median"], 6)


def test_cli_beside_the_dense_options():
    """stripped before the positional arguments are counted, in any order with the --dense-* options"""
    argv = ["prog", "--dense-tile=256", "p1", "--class-weights=median", "p2", "--dense-tta=d4", "--dense-scales=0.75,1", "p3"]
    argv, tile = cli.parse_dense_tile(argv)
    argv, tta = cli.parse_dense_tta(argv)
    argv, scales = cli.parse_dense_scales(argv)
    argv, se = cli.parse_dense_se(argv)
    argv, cw = cli.parse_class_weights(argv, 6)
    assert (argv, tile, tta, scales, se, cw) == (["prog", "p1", "p2", "p3"], 256, "d4", (0.75, 1.0), None, "median")
    # and the other way round: the dense parsers leave the option alone
    argv0 = ["prog", "--class-weights=1,2", "x"]
    assert cli.parse_dense_tile(argv0) == (argv0, None) and cli.parse_dense_scales(argv0) == (argv0, None)


def test_cli_main_reports_a_bad_option_before_anything_else():
    with pytest.raises(SystemExit) as e:
        cli.main(["prog", "--class-weights=1,2,3"], device="cpu")
    assert "--class-weights" in str(e.value) and "6" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main_coffee(["prog", "--class-weights=1,2,3"], device="cpu")
    assert "--class-weights" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main_contest(["prog", "--class-weights=-1,1,1,1,1,1,1"], device="cpu")
    assert "--class-weights" in str(e.value)


# ------------------------------------------------------------------------------------------------- checkpoint
class _FakeNet(object):
    """what save_checkpoint / load_checkpoint touch of a net"""

    def __init__(self, K):
        self.K, self._w, self.state = K, None, {"conv1/weights": np.arange(6, dtype=np.float32), "main_global_step": np.array(0, dtype=np.int64)}

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, d):
        self.state = {k: np.asarray(v) for k, v in d.items()}

    def set_class_weights(self, w):
        self._w = None if w is None else P.check_class_weights(w, self.K)

    @property
    def class_weights(self):
        return None if self._w is None else self._w.copy()


def test_checkpoint_round_trip_of_the_weights(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet(4)
    w = P.check_class_weights(list(P.class_weights([600, 390, 0, 10], "balanced")), 4)
    a.set_class_weights(w)
    loops.save_checkpoint(a, out, 1000, np.zeros(3, np.float32), np.ones(3, np.int32), np.zeros(3, np.int32))
    assert os.path.isfile(out + "class_weights_step_1000.npy") and os.path.isfile(out + "patch_occur_step_1000.npy")
    with np.load(out + "model-1000.npz") as d:
        assert sorted(d.files) == sorted(a.state)            # the model file keeps the TensorFlow variable set: no weights in it
    b = _FakeNet(4)
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-1000")
    text = capsys.readouterr().out                          # a resumed run says in its log that its loss is weighted, and how
    assert "Class weights (restored from " + out + "class_weights_step_1000.npy): weights ['0.555556', '0.854701', '1', '33.3333']" in text
    assert b.class_weights.dtype == np.float32 and b.class_weights.tobytes() == w.tobytes()       # the same bits: the same loss
    np.testing.assert_array_equal(b.state["conv1/weights"], a.state["conv1/weights"])
    c = _FakeNet(4)
    loops.load_checkpoint(c, out + "model-1000.npz")
    assert c.class_weights.tobytes() == w.tobytes()


def test_checkpoint_without_weights_leaves_none(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet(4)
    loops.save_checkpoint(a, out, 7)
    assert not os.path.exists(out + "class_weights_step_7.npy")
    b = _FakeNet(4)
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-7")
    assert b.class_weights is None and "Class weights" not in capsys.readouterr().out
    # a checkpoint of another step's weights is not picked up
    a.set_class_weights([1, 2, 3, 4])
    loops.save_checkpoint(a, out, 8)
    loops.load_checkpoint(b, out + "model-7")
    assert b.class_weights is None


def test_parse_value_is_finite():
    assert all(math.isfinite(v) for v in P.parse_class_weights("1,2,3"))
    assert P.parse_class_weights("balanced") == "balanced"
