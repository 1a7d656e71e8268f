"""Host side of the soft Dice / Tversky term of the training loss: the numpy statement (tests/dice_ref.py) against fp64
autograd of the loss written with torch ops and against central finite differences, the empty-patch and absent-class cases, shard
invariance, the argument domains of the new entry points and of the setter, the command-line option, the checkpoint side file, and
the agreement of include/drs.h, _lib.py and the library's exports.  No GPU: the kernels and the step are held by
tests/test_gpu_dice_loss.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from drs_amd import _lib, cli, loops, patches as P

import dice_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the reference
def _case(seed=0, B=3, n=23, K=4):
    """patch 0: every class; patch 1: class 2 absent, a few labels >= K, a loss mask with holes; patch 2: no pixel in the loss"""
    rng = np.random.default_rng(seed)
    lg = rng.normal(size=(B, n, K)) * 2.0
    y = rng.integers(0, K, size=(B, n))
    y[0, :K] = np.arange(K)
    y[1][y[1] == 2] = 0
    y[1, :3] = (K, 200, 255)
    lm = (rng.random((B, n)) < 0.8).astype(np.uint8)
    lm[0] = 1
    lm[2] = 0
    return lg, y, lm


def _torch_loss(t, y, lm, K, lam, alpha, beta, smooth, inv_n):
    """the loss written with torch ops, patch by patch, not the closed form"""
    total = 0.0
    for b in range(t.shape[0]):
        ok = torch.as_tensor((y[b] < K) & (lm[b] != 0))
        nb = int(ok.sum())
        if nb == 0:
            continue
        p = torch.softmax(t[b][ok], dim=1)
        oh = torch.nn.functional.one_hot(torch.as_tensor(y[b])[ok], K).to(torch.float64)
        tp = (p * oh).sum(dim=0)
        fp = (p * (1.0 - oh)).sum(dim=0)
        fn = ((1.0 - p) * oh).sum(dim=0)
        tversky = (tp + smooth) / (tp + alpha * fp + beta * fn + smooth)
        total = total + nb * (lam / K) * (1.0 - tversky).sum()
    return inv_n * total


@pytest.mark.parametrize("alpha,beta", [(0.5, 0.5), (0.3, 0.7), (0.0, 1.0), (1.0, 0.0)])
def test_closed_form_against_autograd_and_finite_differences(alpha, beta):
    K, lam, smooth = 4, 1.5, 1.0
    lg, y, lm = _case()
    inv_n = 1.0 / 57.0              # any normaliser: the step's global one
    ref = DR.dice(lg, y, K, lam, alpha, beta, smooth, loss_mask=lm, inv_n=inv_n)
    t = torch.tensor(lg, dtype=torch.float64, requires_grad=True)
    loss = _torch_loss(t, y, lm, K, lam, alpha, beta, smooth, inv_n)
    loss.backward()
    assert abs(ref["loss"] - float(loss.detach())) < 1e-14 * max(1.0, abs(ref["loss"]))
    np.testing.assert_allclose(ref["grad"], t.grad.numpy(), rtol=0, atol=1e-15)
    assert ref["loss"] > 0 and np.abs(ref["grad"]).max() > 1e-4
    # central differences on a sample of logits of every patch
    rng = np.random.default_rng(1)
    h = 1e-6
    for _ in range(24):
        b, i, k = rng.integers(0, lg.shape[0]), rng.integers(0, lg.shape[1]), rng.integers(0, K)
        up, dn = lg.copy(), lg.copy()
        up[b, i, k] += h
        dn[b, i, k] -= h
        fd = (DR.dice(up, y, K, lam, alpha, beta, smooth, lm, inv_n)["loss"] - DR.dice(dn, y, K, lam, alpha, beta, smooth, lm, inv_n)["loss"]) / (2 * h)
        assert abs(fd - ref["grad"][b, i, k]) < 1e-8, (b, i, k)
    # a pixel's logit gradients sum to zero (softmax), and pixels outside the loss get exact zeros
    assert np.abs(ref["grad"].sum(axis=2)).max() < 1e-16
    assert not ref["grad"][~ref["inl"]].any() and (~ref["inl"]).sum() > lg.shape[1]


def test_empty_patch_and_absent_class():
    K = 4
    lg, y, lm = _case()
    ref = DR.dice(lg, y, K, 2.0, 0.3, 0.7, 1.0, loss_mask=lm)
    # patch 2 has no pixel in the loss: T = 1 for every class, zero coefficients, no loss, no gradient
    assert ref["n"][2] == 0 and (ref["T"][2] == 1.0).all() and not ref["g_in"][2].any() and not ref["g_out"][2].any()
    assert ref["patch_loss"][2] == 0.0 and not ref["grad"][2].any()
    # patch 1 lacks class 2: N = TP = 0, T = eps / (alpha SP + eps) < 1, and the class still pushes its probability down everywhere
    assert ref["cnt"][1, 2] == 0 and ref["tp"][1, 2] == 0 and ref["sp"][1, 2] > 0
    assert ref["T"][1, 2] == 1.0 / (0.3 * ref["sp"][1, 2] + 1.0) and ref["g_out"][1, 2] > 0
    # labels >= K are outside the loss and N counts the rest exactly
    assert ref["cnt"].sum() == ref["inl"].sum() and not ref["inl"][1, :3].any()
    # lam times the mean over patches and classes of 1 - T when every pixel is in the loss
    full = DR.dice(lg, np.minimum(y, K - 1), K, 2.0)
    assert abs(full["loss"] - 2.0 * (1.0 - full["T"]).mean()) < 1e-15


def test_shard_invariance_in_the_reference():
    """the loss and gradient of B = 4 are the sums over its two halves, each with the global inv_n: what lets a sharded batch train as
    the whole one does with no collective"""
    K = 3
    rng = np.random.default_rng(3)
    lg = rng.normal(size=(4, 31, K))
    y = rng.integers(0, K + 1, size=(4, 31))            # (a few labels == K: outside the loss)
    lm = (rng.random((4, 31)) < 0.7).astype(np.uint8)
    inv_n = 1.0 / float(DR.in_loss(y, K, lm).sum())
    whole = DR.dice(lg, y, K, 1.0, 0.3, 0.7, 1.0, lm, inv_n)
    halves = [DR.dice(lg[s], y[s], K, 1.0, 0.3, 0.7, 1.0, lm[s], inv_n) for s in (slice(0, 2), slice(2, 4))]
    assert abs(whole["loss"] - (halves[0]["loss"] + halves[1]["loss"])) < 1e-15
    np.testing.assert_array_equal(whole["grad"], np.concatenate([h["grad"] for h in halves]))
    np.testing.assert_array_equal(whole["g_in"], np.concatenate([h["g_in"] for h in halves]))


# ------------------------------------------------------------------------------------------------- the entry points' checks
OK, ERR_ARG, ERR_HIP = 0, 1, 2
p0, p1, p2, p3, p4, p5, p6, p7, p8, p9 = [0x10000 + 0x1000 * i for i in range(10)]     # dummy device pointers: host code never dereferences them
NAN, INFTY = float("nan"), float("inf")
WC6 = (C.c_float * 6)(1, 2, 0, 1, 1, 1)
WC_BAD = (C.c_float * 6)(1, 2, -1, 1, 1, 1)
ROWS = {
    "drs_patch_dice_coeffs": (
        [("logits", p0), ("labels", p1), ("loss_mask", p2), ("B", 3), ("S", 21), ("K", 6), ("lam", 1.0), ("alpha", 0.5), ("beta", 0.5),
         ("smooth", 1.0), ("stats_out", p3), ("coef_out", p4), ("patch_loss_out", p5)],
        [dict(logits=None), dict(labels=None), dict(coef_out=None), dict(patch_loss_out=None), dict(B=0), dict(S=0), dict(B=-3), dict(S=-21),
         dict(B=1 << 12, S=64), dict(B=1, S=4096), dict(B=1 << 20, S=1 << 20), dict(K=0), dict(K=9), dict(K=-1), dict(lam=0.0), dict(lam=-1.0),
         dict(lam=64.5), dict(lam=NAN), dict(lam=INFTY), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=NAN), dict(beta=-0.01),
         dict(beta=1.01), dict(beta=NAN), dict(beta=INFTY), dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=float((1 << 20) + 1)),
         dict(smooth=NAN), dict(smooth=INFTY)],
        [dict(loss_mask=None), dict(stats_out=None), dict(lam=64.0), dict(lam=1e-6), dict(alpha=0.0, beta=1.0), dict(alpha=1.0, beta=0.0),
         dict(smooth=float(1 << 20)), dict(smooth=1e-9), dict(K=1), dict(K=8), dict(B=1, S=4095), dict(B=1, S=1)]),
    "drs_classifier_loss_dice": (
        [("feat", p0), ("B", 2), ("S", 13), ("P", 0), ("ld", 256), ("coff", 0), ("C", 256), ("K", 6), ("w", p1), ("bias", p2), ("labels", p3),
         ("loss_mask", None), ("acc_mask", None), ("inv_n", 1.0 / 338), ("class_weights", WC6), ("focal_gamma", 2.0), ("pixel_weight", p4),
         ("dice_coef", p9), ("logits", None), ("pred", None), ("gfeat", p5), ("ld_g", 256), ("coff_g", 0), ("dw_partial", p6),
         ("db_partial", p7), ("loss_partial", p8), ("conf", None)],
        [dict(feat=None), dict(w=None), dict(bias=None), dict(K=0), dict(K=9), dict(C=32), dict(C=100), dict(C=512), dict(B=0), dict(S=0),
         dict(P=-1), dict(inv_n=NAN), dict(inv_n=-1.0), dict(focal_gamma=-0.5), dict(focal_gamma=8.5), dict(focal_gamma=NAN),
         dict(class_weights=WC_BAD), dict(loss_partial=None), dict(dw_partial=None), dict(db_partial=None), dict(labels=None),
         dict(ld=258), dict(coff=2), dict(ld_g=258), dict(B=1 << 12, S=64), dict(dice_coef=p9 + 4)],
        [dict(dice_coef=None), dict(pixel_weight=None), dict(class_weights=None), dict(focal_gamma=0.0),
         dict(class_weights=None, focal_gamma=0.0, pixel_weight=None), dict(labels=None, gfeat=None), dict(dice_coef=p9 + 8)]),
    "drs_dice_loss_add": (
        [("patch_loss", p0), ("B", 3), ("loss_sum", p1)],
        [dict(patch_loss=None), dict(loss_sum=None), dict(B=0), dict(B=-1)],
        [dict(B=1), dict(B=1 << 20)]),
}


def _call(lib, name, args, change=None):
    a = dict(args)
    assert not change or set(change) <= set(a), (name, change)
    a.update(change or {})
    return getattr(lib, name)(*[a[k] for k, _ in args], None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the in-domain rows would launch kernels on dummy pointers: CPU machines only")
@pytest.mark.parametrize("name", sorted(ROWS))
def test_abi_rows(name):
    """in the manner of tests/test_abi_contract.py: the baseline and every in-domain edge pass validation (what comes back is the
    launch's status), every single violation returns exactly DRS_ERR_ARG"""
    lib = _lib.load()
    args, bad, good = ROWS[name]
    for change in [None] + good:
        rc = _call(lib, name, args, change)
        assert rc != ERR_ARG and rc in (OK, ERR_HIP), (name, change, rc)
    wrong = [(change, rc) for change in bad for rc in [_call(lib, name, args, change)] if rc != ERR_ARG]
    assert not wrong, "%s: not DRS_ERR_ARG for %r" % (name, wrong)


def test_violations_are_rejected_on_any_machine():
    """the rejections alone launch nothing, so they also run where a GPU is present"""
    lib = _lib.load()
    for name in sorted(ROWS):
        args, bad, _ = ROWS[name]
        wrong = [(change, rc) for change in bad for rc in [_call(lib, name, args, change)] if rc != ERR_ARG]
        assert not wrong, "%s: not DRS_ERR_ARG for %r" % (name, wrong)


def test_setter_domain_getter_and_buffers():
    lib = _lib.load()
    h = C.c_void_p()
    _lib.call("drs_net_create", b"dilated_grsl", 5, 6, 0.005, 2, 17, 0, 0.5, C.byref(h))
    try:
        v = [C.c_double(-7) for _ in range(4)]
        get = lambda: (lib.drs_net_get_dice(h, *[C.byref(x) for x in v]), tuple(x.value for x in v))   # noqa: E731
        assert get() == (OK, (0.0, 0.5, 0.5, 1.0))                                  # never set: off, the defaults
        for bad in ((-0.1, 0.5, 0.5, 1.0), (64.5, 0.5, 0.5, 1.0), (NAN, 0.5, 0.5, 1.0), (INFTY, 0.5, 0.5, 1.0), (1.0, -0.1, 0.5, 1.0),
                    (1.0, 1.1, 0.5, 1.0), (1.0, NAN, 0.5, 1.0), (1.0, 0.5, -0.1, 1.0), (1.0, 0.5, 1.1, 1.0), (1.0, 0.5, NAN, 1.0),
                    (1.0, 0.5, 0.5, 0.0), (1.0, 0.5, 0.5, -1.0), (1.0, 0.5, 0.5, 2.0 ** 20 + 1), (1.0, 0.5, 0.5, NAN), (1.0, 0.5, 0.5, INFTY),
                    (0.0, 0.5, 0.5, 0.0), (0.0, 2.0, 0.5, 1.0)):
            assert lib.drs_net_set_dice(h, *bad) == ERR_ARG, bad
        assert get() == (OK, (0.0, 0.5, 0.5, 1.0))                                  # a rejected call changes nothing
        for good in ((1.0, 0.5, 0.5, 1.0), (64.0, 0.0, 1.0, 2.0 ** 20), (1e-3, 1.0, 0.0, 1e-6), (0.0, 0.3, 0.7, 2.0)):
            assert lib.drs_net_set_dice(h, *good) == OK
            assert get() == (OK, good)
        assert lib.drs_net_get_dice(h, None, None, None, None) == OK
        assert lib.drs_net_set_dice(None, 1.0, 0.5, 0.5, 1.0) == ERR_ARG and lib.drs_net_get_dice(None, None, None, None, None) == ERR_ARG
        # the buffers the step writes the coefficients and the patches' terms into: b_max K 2 floats, b_max doubles
        name, nb, dt = C.create_string_buffer(64), C.c_size_t(), C.c_int()
        info = {}
        for i in range(_lib.query("drs_net_num_buffers", h)):
            _lib.call("drs_net_buffer_info", h, i, name, 64, C.byref(nb), C.byref(dt))
            info[name.value.decode()] = nb.value
        assert info["dice_coef"] == 4 * 2 * 6 * 2 and info["dice_loss"] == 8 * 2
    finally:
        lib.drs_net_destroy(h)


def test_timing_kinds_are_unchanged():
    assert _lib.query("drs_net_num_timing_kinds") == 15


# ------------------------------------------------------------------------------------------------- the quadruple
def test_check_dice():
    assert P.check_dice(1) == (1.0, 0.5, 0.5, 1.0) and P.check_dice((2.5,)) == (2.5, 0.5, 0.5, 1.0)
    assert P.check_dice((1, 0.3, 0.7)) == (1.0, 0.3, 0.7, 1.0) and P.check_dice([64, 0, 1, 2 ** 20]) == (64.0, 0.0, 1.0, float(2 ** 20))
    assert P.check_dice((0, 0.5, 0.5, 1)) == (0.0, 0.5, 0.5, 1.0) and P.check_dice((np.float32(2), np.float64(1), np.int64(0), 1e-3)) == (2.0, 1.0, 0.0, 1e-3)
    for bad in ((), (1, 0.5), (1, 2, 3, 4, 5), "1", (True,), (1, "0.5", 0.5), -0.5, 64.5, NAN, INFTY, (1, -0.1, 0.5), (1, 0.5, 1.1), (1, NAN, 0.5),
                (1, 0.5, 0.5, 0), (1, 0.5, 0.5, -1), (1, 0.5, 0.5, 2 ** 20 + 1), (1, 0.5, 0.5, NAN), (1, 0.5, 0.5, True), None):
        with pytest.raises(ValueError):
            P.check_dice(bad)


def test_parse_dice():
    assert P.parse_dice("1") == (1.0, 0.5, 0.5, 1.0) and P.parse_dice("0.5,0.3,0.7") == (0.5, 0.3, 0.7, 1.0)
    assert P.parse_dice("2,0.3,0.7,1e-3") == (2.0, 0.3, 0.7, 1e-3) and P.parse_dice("0") == (0.0, 0.5, 0.5, 1.0)
    for bad in ("", " 1", "1 ", "1,", ",0.5", "1,0.5", "1,0.5,0.5,", "1,0.5,0.5,1,2", "one", "1,x,0.5", "65", "-1", "1,2,0.5", "1,0.5,-1", "1,0.5,0.5,0",
                "nan", "inf", "1, 0.5,0.5"):
        with pytest.raises(ValueError):
            P.parse_dice(bad)


# ------------------------------------------------------------------------------------------------- command line
def test_cli_good_forms():
    base = ["prog", "a", "b"]
    assert cli.parse_dice(base) == (base, None)
    assert cli.parse_dice(base + ["--dice-weight=1"]) == (base, (1.0, 0.5, 0.5, 1.0))
    assert cli.parse_dice(["prog", "--dice-weight=0.5,0.3,0.7", "a", "b"]) == (base, (0.5, 0.3, 0.7, 1.0))
    assert cli.parse_dice(["prog", "a", "--dice-weight=2,0.3,0.7,0.01", "b"]) == (base, (2.0, 0.3, 0.7, 0.01))
    assert cli.parse_dice(["prog", "a", "--dice-weight=0", "b"]) == (base, (0.0, 0.5, 0.5, 1.0))


@pytest.mark.parametrize("arg", ["--dice-weight", "--dice-weight=", "--dice-weight=-1", "--dice-weight=nan", "--dice-weight=65", "--dice-weight=one",
                                 "--dice-weight=1,0.5", "--dice-weight=1,2,0.5", "--dice-weight=1,0.5,0.5,0", "--dice-weight= 2",
                                 "--dice-weight=1,2,3,4,5"])
def test_cli_bad_forms_name_the_option_and_the_form(arg):
    with pytest.raises(ValueError) as e:
        cli.parse_dice(["prog", "a", arg])
    msg = str(e.value)
    assert "--dice-weight=lam[,alpha,beta[,smooth]]" in msg and "[0, 64]" in msg and "[0, 1]" in msg


def test_cli_twice_is_refused():
    with pytest.raises(ValueError, match="--dice-weight given more than once"):
        cli.parse_dice(["prog", "--dice-weight=2", "x", "--dice-weight=2"])


def test_cli_beside_the_other_loss_options():
    argv = ["prog", "p1", "--focal-gamma=2", "--dice-weight=1,0.3,0.7", "--boundary-weight=10,3", "--class-weights=median", "p2"]
    argv, cw = cli.parse_class_weights(argv, 6)
    argv, g = cli.parse_focal_gamma(argv)
    argv, bw = cli.parse_boundary_weight(argv)
    argv, dc = cli.parse_dice(argv)
    assert (argv, cw, g, bw, dc) == (["prog", "p1", "p2"], "median", 2.0, (10.0, 3.0, 9), (1.0, 0.3, 0.7, 1.0))
    argv0 = ["prog", "--dice-weight=2", "x"]
    assert cli.parse_focal_gamma(argv0) == (argv0, None) and cli.parse_boundary_weight(argv0) == (argv0, None)


def test_cli_main_reports_a_bad_option_in_all_three_flavours():
    for main in (cli.main, cli.main_coffee, cli.main_contest):
        with pytest.raises(SystemExit) as e:
            main(["prog", "--dice-weight=-2"], device="cpu")
        assert "--dice-weight" in str(e.value) and "[0, 64]" in str(e.value)
        with pytest.raises(SystemExit) as e:
            main(["prog", "--dice-weight=1", "--dice-weight=2"], device="cpu")
        assert "--dice-weight given more than once" in str(e.value)
        with pytest.raises(SystemExit) as e:                # a good value is taken out of argv: what is left is too short, the usage line
            main(["prog", "--dice-weight=1,0.3,0.7"], device="cpu")
        assert str(e.value).startswith("Usage: ")


def test_cli_outside_training_is_refused():
    isprs = ["prog"] + ["x"] * 15
    for process in ("validate_test", "generate_final_maps"):
        with pytest.raises(SystemExit) as e:
            cli.main(isprs + [process, "--dice-weight=2"], device="cpu")
        assert str(e.value) == "--dice-weight applies to the training process only"
    contest = ["prog", "--dice-weight=2"] + ["x"] * 13
    with pytest.raises(SystemExit) as e:
        cli.main_contest(contest + ["test"], device="cpu")
    assert "--dice-weight applies to the train operation only" in str(e.value)


def test_cli_flag_reaches_the_loops():
    from drs_amd import loops_indexed as LI
    for fn in (loops.train, LI.train):
        assert inspect.signature(fn).parameters["dice"].default is None
    assert inspect.getsource(cli).count("dice=dice") == 3


# ------------------------------------------------------------------------------------------------- checkpoint
class _FakeNet(object):
    """what save_checkpoint / load_checkpoint / setup_dice touch of a net"""

    def __init__(self):
        self._d = None
        self.state = {"conv1/weights": np.arange(6, dtype=np.float32), "main_global_step": np.array(0, dtype=np.int64)}

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, d):
        self.state = {k: np.asarray(v) for k, v in d.items()}

    class_weights, focal_gamma, boundary_weight = None, 0.0, None

    def set_dice(self, d):
        self._d = None if d is None else P.check_dice(d)

    @property
    def dice(self):
        return None if self._d is None or self._d[0] == 0.0 else self._d


def test_checkpoint_round_trip_of_the_quadruple(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet()
    a.set_dice((0.1, 0.3, 0.7, 2.5))
    loops.save_checkpoint(a, out, 1000, np.zeros(3, np.float32), np.ones(3, np.int32), np.zeros(3, np.int32))
    assert os.path.isfile(out + "dice_step_1000.npy") and os.path.isfile(out + "patch_occur_step_1000.npy")
    assert not os.path.exists(out + "focal_gamma_step_1000.npy") and not os.path.exists(out + "boundary_weight_step_1000.npy")
    side = np.load(out + "dice_step_1000.npy")
    assert side.dtype == np.float64 and side.tolist() == [0.1, 0.3, 0.7, 2.5]
    with np.load(out + "model-1000.npz") as d:
        assert sorted(d.files) == sorted(a.state)            # the model file keeps the TensorFlow variable set
    b = _FakeNet()
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-1000")
    text = capsys.readouterr().out
    assert "Dice term (restored from " + out + "dice_step_1000.npy): lambda 0.1 alpha 0.3 beta 0.7 smooth 2.5" in text
    assert b.dice == a.dice == (0.1, 0.3, 0.7, 2.5)          # the same doubles: the same loss


def test_checkpoint_without_the_option_leaves_none(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet()
    loops.save_checkpoint(a, out, 7)
    a.set_dice((0, 0.3, 0.7))
    loops.save_checkpoint(a, out, 7)
    assert not os.path.exists(out + "dice_step_7.npy")       # lam = 0 is unset
    b = _FakeNet()
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-7")
    assert b.dice is None and "Dice term" not in capsys.readouterr().out
    a.set_dice(5)
    loops.save_checkpoint(a, out, 8)
    loops.load_checkpoint(b, out + "model-7")                # another step's quadruple is not picked up
    assert b.dice is None


def test_setup_dice_overrides_and_says_so():
    from drs_amd.net import NoComm
    lines = []
    net = _FakeNet()
    assert loops.setup_dice(net, 0, NoComm(), lines.append) == (0.0, 0.5, 0.5, 1.0) and lines == [] and net.dice is None
    assert loops.setup_dice(net, (1, 0.3, 0.7), NoComm(), lines.append) == (1.0, 0.3, 0.7, 1.0) and net.dice == (1.0, 0.3, 0.7, 1.0)
    assert len(lines) == 1 and "Dice term: lambda 1 alpha 0.3 beta 0.7 smooth 1" in lines[0] and "replacing" not in lines[0]
    loops.setup_dice(net, 2, NoComm(), lines.append)
    assert len(lines) == 2 and "lambda 2 alpha 0.5 beta 0.5 smooth 1" in lines[1]
    assert "replacing the quadruple restored from the checkpoint, lambda 1 alpha 0.3 beta 0.7 smooth 1" in lines[1]
    loops.setup_dice(net, 0, NoComm(), lines.append)
    assert net.dice is None and len(lines) == 3 and "lambda 0 (off" in lines[2] and "replacing" in lines[2]
    with pytest.raises(ValueError):
        loops.setup_dice(net, 65, NoComm(), lines.append)

    class TwoRanks(NoComm):
        def agree(self, values, what):
            self.seen = (list(values), what)
    comm = TwoRanks()
    loops.setup_dice(net, (1, 0.3, 0.7, 1), comm, lines.append)
    assert comm.seen == (np.asarray([1.0, 0.3, 0.7, 1.0], dtype=np.float64).view(np.uint32).tolist(), "dice term")


# ------------------------------------------------------------------------------------------------- header, signatures, exports
def test_header_lib_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    new = ("drs_patch_dice_coeffs", "drs_classifier_loss_dice", "drs_dice_loss_add", "drs_net_set_dice", "drs_net_get_dice")
    exported = set(re.findall(r" T (drs_[a-z0-9_]+)$", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                                                                        check=True).stdout, flags=re.M))
    lib = _lib.load()
    for name in new:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", hdr, flags=re.M)
        assert m, name
        nargs = len([a for a in m.group(1).replace("\n", " ").split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, (name, nargs)
        assert name in exported and hasattr(lib, name)
    # the op-level entry points sit in the training-level part at the end of the header, after the boundary-weight ones
    step = hdr.index("Step level: the reference's three `sess.run` call shapes")
    assert hdr.index("int drs_patch_dice_coeffs(") > hdr.index("int drs_classifier_loss_pixel(") > step
    assert hdr.index("int drs_classifier_loss_dice(") > hdr.index(" * Training level: soft Dice / Tversky term (opt-in") > hdr.index("int drs_classifier_loss_pixel(")
    assert step < hdr.index("int drs_net_set_dice(") < hdr.index("Whole-map level")
    # the Dice form is the pixel form plus one pointer
    pixel, dice = _lib.SIGNATURES["drs_classifier_loss_pixel"][1], _lib.SIGNATURES["drs_classifier_loss_dice"][1]
    assert dice[:17] == pixel[:17] and dice[18:] == pixel[17:] and dice[17] is C.c_void_p
