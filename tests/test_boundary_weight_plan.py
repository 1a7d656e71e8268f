"""Host side of the boundary-weighted training loss: the numpy statement (tests/boundary_weight_ref.py) against
hand-worked maps, the argument domains of the two op-level entry points and of the setter, the command-line option, the checkpoint
side file, and the agreement of include/drs.h, _lib.py and the library's exports.  No GPU: the kernels and the step are held by
tests/test_gpu_boundary_weight.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from drs_amd import _lib, cli, loops, patches as P

import boundary_weight_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = BR.INF


# ------------------------------------------------------------------------------------------------- the reference
def test_ref_a_straight_edge_gives_the_squares():
    S = 9
    lab = np.zeros((1, S, S), dtype=np.uint8)
    lab[:, :, 5:] = 3                              # columns 0..4 class 0, 5..8 class 3
    d2 = BR.boundary_d2(lab, None, 16)
    want = np.asarray([25, 16, 9, 4, 1, 1, 4, 9, 16])
    assert (d2[0] == want[None, :]).all()
    d2 = BR.boundary_d2(lab, None, 2)               # the window cuts the tail: beyond R there is no other class
    want = np.asarray([INF, INF, INF, 4, 1, 1, 4, INF, INF])
    assert (d2[0] == want[None, :]).all()
    w, _ = BR.boundary_weight(lab, None, 2, 10.0, 1.0 / 32.0)
    assert (w[0, :, :3] == 1.0).all() and (w[0, :, 7:] == 1.0).all()
    np.testing.assert_allclose(w[0, 0, 3:7], 1.0 + 10.0 * np.exp(-np.asarray([4, 1, 1, 4]) / 32.0), rtol=0, atol=1e-15)
    assert (BR.boundary_d2_loops(lab, None, 2) == d2).all()


def test_ref_a_single_pixel_of_another_class():
    S = 7
    lab = np.full((1, S, S), 2, dtype=np.uint8)
    lab[0, 3, 4] = 5
    d2 = BR.boundary_d2(lab, None, 3)
    yy, xx = np.mgrid[0:S, 0:S]
    dy, dx = yy - 3, xx - 4
    want = np.where((np.abs(dy) <= 3) & (np.abs(dx) <= 3), dy * dy + dx * dx, INF)
    want[3, 4] = 1                                  # the pixel itself: its four neighbours carry the other byte
    assert (d2[0] == want).all()
    assert d2[0, 0, 0] == INF and d2[0, 0, 1] == 18 and d2[0, 6, 6] == 13        # (0, 0): dx = 4 > R; the window is a square, not a disc


def test_ref_an_invalid_stripe_between_two_classes():
    """the stripe itself weighs 1, never counts as "different", and does not hide the class behind it"""
    S = 8
    lab = np.zeros((1, S, S), dtype=np.uint8)
    lab[:, :, 4:] = 1
    lab[:, :, 3:5] = 0                              # what the crop kernel writes under mask 0: label 0
    valid = np.ones((1, S, S), dtype=np.uint8)
    valid[:, :, 3:5] = 0
    d2 = BR.boundary_d2(lab, valid, 4)
    want = np.asarray([INF, 16, 9, INF, INF, 9, 16, INF])       # columns 0 1 2 | 3 4 invalid | 5 6 7; column 0 -> 5 is dx = 5 > R
    assert (d2[0] == want[None, :]).all()
    assert (BR.boundary_d2_loops(lab, valid, 4) == d2).all()
    # without the validity map the fill draws contours of its own: the rule with valid = NULL
    d2n = BR.boundary_d2(lab, None, 4)
    assert (d2n[0, :, 4] == 1).all() and (d2n[0, :, 5] == 1).all() and (d2n[0, :, 3] == 4).all()
    w, _ = BR.boundary_weight(lab, valid, 4, 10.0, 0.05)
    assert (w[0, :, 3:5] == 1.0).all() and (w[0, :, 0] == 1.0).all() and (w[0, :, 2] > 1.0).all()


def test_ref_patches_and_rows_are_independent():
    lab = np.zeros((2, 5, 5), dtype=np.uint8)
    lab[1] = 4                                      # two uniform patches with different labels: nothing anywhere
    assert (BR.boundary_d2(lab, None, 16) == INF).all()
    lab = np.zeros((1, 4, 4), dtype=np.uint8)
    lab[0, 1, 0] = 1                                # row 0 ends in class 0, row 1 begins in class 1: (0, 3) is 3 columns away, not 1
    d2 = BR.boundary_d2(lab, None, 16)
    assert d2[0, 0, 3] == 10 and d2[0, 1, 0] == 1 and d2[0, 0, 0] == 1
    assert (BR.boundary_d2_loops(lab, None, 16) == d2).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ref_vectorised_equals_the_loops(seed):
    rng = np.random.default_rng(seed)
    B, S, R = 2, 11, 1 + 3 * seed
    lab = rng.integers(0, 3, size=(B, S, S)).astype(np.uint8) * (rng.random((B, S, S)) < 0.3)
    valid = (rng.random((B, S, S)) < 0.8).astype(np.uint8)
    for v in (None, valid):
        assert (BR.boundary_d2(lab, v, R) == BR.boundary_d2_loops(lab, v, R)).all()
    assert (BR.d2_u16(BR.boundary_d2(lab, valid, R)) <= 65535).all() and BR.d2_u16(np.asarray([INF, 70000, 5])).tolist() == [65535, 65535, 5]


def test_ref_loss_with_a_map_against_autograd():
    rng = np.random.default_rng(5)
    M, K = 40, 4
    lg = rng.normal(size=(M, K)) * 2
    y = rng.integers(0, K, size=M)
    wc = np.asarray([0.5, 2.0, 1.0, 0.0])
    pw = 1.0 + 10.0 * rng.random(M) * (rng.random(M) < 0.5)
    for gamma in (0.0, 2.0):
        t = torch.tensor(lg, dtype=torch.float64, requires_grad=True)
        yy = torch.as_tensor(y, dtype=torch.long)
        logp = torch.log_softmax(t, dim=1).gather(1, yy[:, None])[:, 0]
        term = torch.as_tensor(pw) * torch.as_tensor(wc)[yy] * (1.0 - torch.exp(logp)) ** gamma * (-logp)
        term.sum().backward()
        ref = BR.pixel_weighted_closed_form(lg, y, wc, gamma, pw)
        np.testing.assert_allclose(ref["term"], term.detach().numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ref["grad"], t.grad.numpy(), rtol=1e-11, atol=1e-13)


# ------------------------------------------------------------------------------------------------- the entry points' checks
OK, ERR_ARG, ERR_HIP = 0, 1, 2
p0, p1, p2, p3, p4, p5, p6, p7, p8, p9 = [0x10000 + 0x1000 * i for i in range(10)]     # dummy device pointers: host code never dereferences them
NAN, INFTY = float("nan"), float("inf")
WC6 = (C.c_float * 6)(1, 2, 0, 1, 1, 1)
WC_BAD = (C.c_float * 6)(1, 2, -1, 1, 1, 1)
ROWS = {
    "drs_patch_boundary_weight": (
        [("lab", p0), ("valid", p1), ("B", 3), ("S", 21), ("R", 4), ("a", 10.0), ("c", 1.0 / 32.0), ("d2_out", p2), ("weight_out", p3)],
        [dict(B=0), dict(S=0), dict(B=-3), dict(S=-21), dict(B=1 << 12, S=64), dict(B=1, S=4096), dict(B=1 << 20, S=1 << 20),
         dict(R=0), dict(R=17), dict(R=-4), dict(a=-1.0000001), dict(a=64.5), dict(a=NAN), dict(a=INFTY), dict(a=-INFTY),
         dict(c=0.0), dict(c=-0.1), dict(c=NAN), dict(c=INFTY), dict(lab=None), dict(weight_out=None)],
        [dict(valid=None), dict(d2_out=None), dict(a=-1.0), dict(a=64.0), dict(a=0.0), dict(R=1), dict(R=16), dict(B=1, S=4095), dict(B=1, S=1)]),
    "drs_classifier_loss_pixel": (
        [("feat", p0), ("B", 2), ("S", 13), ("P", 0), ("ld", 256), ("coff", 0), ("C", 256), ("K", 6), ("w", p1), ("bias", p2), ("labels", p3),
         ("loss_mask", None), ("acc_mask", None), ("inv_n", 1.0 / 338), ("class_weights", WC6), ("focal_gamma", 2.0), ("pixel_weight", p4),
         ("logits", None), ("pred", None), ("gfeat", p5), ("ld_g", 256), ("coff_g", 0), ("dw_partial", p6), ("db_partial", p7),
         ("loss_partial", p8), ("conf", None)],
        [dict(feat=None), dict(w=None), dict(bias=None), dict(K=0), dict(K=9), dict(C=32), dict(C=100), dict(C=512), dict(B=0), dict(S=0),
         dict(P=-1), dict(inv_n=NAN), dict(inv_n=-1.0), dict(focal_gamma=-0.5), dict(focal_gamma=8.5), dict(focal_gamma=NAN),
         dict(class_weights=WC_BAD), dict(loss_partial=None), dict(dw_partial=None), dict(db_partial=None), dict(labels=None),
         dict(ld=258), dict(coff=2), dict(ld_g=258), dict(B=1 << 12, S=64)],
        [dict(pixel_weight=None), dict(class_weights=None), dict(focal_gamma=0.0), dict(class_weights=None, focal_gamma=0.0),
         dict(labels=None, gfeat=None)]),
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


def test_setter_domain_and_getter():
    lib = _lib.load()
    h = C.c_void_p()
    _lib.call("drs_net_create", b"dilated_grsl", 5, 6, 0.005, 2, 17, 0, 0.5, C.byref(h))
    try:
        a, sigma, R = C.c_double(-7), C.c_double(-7), C.c_int(-7)
        assert lib.drs_net_get_boundary_weight(h, C.byref(a), C.byref(sigma), C.byref(R)) == OK
        assert (a.value, sigma.value, R.value) == (0.0, 4.0, 12)                     # never set: off, the defaults
        for bad in ((-1.5, 4.0, 12), (64.5, 4.0, 12), (NAN, 4.0, 12), (INFTY, 4.0, 12), (1.0, 0.0, 12), (1.0, -1.0, 12), (1.0, 64.5, 12),
                    (1.0, NAN, 12), (1.0, INFTY, 12), (1.0, 4.0, 0), (1.0, 4.0, 17), (1.0, 4.0, -1), (0.0, 0.0, 12), (0.0, 4.0, 0)):
            assert lib.drs_net_set_boundary_weight(h, *bad) == ERR_ARG, bad
        assert lib.drs_net_get_boundary_weight(h, C.byref(a), C.byref(sigma), C.byref(R)) == OK
        assert (a.value, sigma.value, R.value) == (0.0, 4.0, 12)                     # a rejected call changes nothing
        for good in ((10.0, 4.0, 12), (-1.0, 64.0, 16), (64.0, 1e-3, 1), (0.0, 2.0, 6)):
            assert lib.drs_net_set_boundary_weight(h, *good) == OK
            assert lib.drs_net_get_boundary_weight(h, C.byref(a), C.byref(sigma), C.byref(R)) == OK
            assert (a.value, sigma.value, R.value) == good
        assert lib.drs_net_get_boundary_weight(h, None, None, None) == OK
        assert lib.drs_net_set_boundary_weight(None, 1.0, 4.0, 12) == ERR_ARG and lib.drs_net_get_boundary_weight(None, None, None, None) == ERR_ARG
        # the buffer the step writes the map into: after the existing entries, b_max * s_max^2 floats
        name, nb, dt = C.create_string_buffer(64), C.c_size_t(), C.c_int()
        n = _lib.query("drs_net_num_buffers", h)
        names = []
        for i in range(n):
            _lib.call("drs_net_buffer_info", h, i, name, 64, C.byref(nb), C.byref(dt))
            names.append(name.value.decode())
        assert names[-1] == "pixel_weight" and names[-2] == "loss_mask" and (nb.value, dt.value) == (4 * 2 * 17 * 17, 0)
    finally:
        lib.drs_net_destroy(h)


def test_timing_kinds_are_unchanged():
    assert _lib.query("drs_net_num_timing_kinds") == 15


# ------------------------------------------------------------------------------------------------- the triple
def test_check_boundary_weight():
    assert P.check_boundary_weight(10) == (10.0, 4.0, 12) and P.check_boundary_weight((2.5,)) == (2.5, 4.0, 12)
    assert P.check_boundary_weight((1, 1.5)) == (1.0, 1.5, 5) and P.check_boundary_weight((1, 8)) == (1.0, 8.0, 16)
    assert P.check_boundary_weight((1, 0.1)) == (1.0, 0.1, 1) and P.check_boundary_weight([-1, 64, 16]) == (-1.0, 64.0, 16)
    assert P.check_boundary_weight((0, 4, 3)) == (0.0, 4.0, 3) and P.check_boundary_weight((np.float32(2), np.float64(3), np.int64(7))) == (2.0, 3.0, 7)
    assert P.check_boundary_weight((2, 3, 7.0)) == (2.0, 3.0, 7)
    for bad in ((), (1, 2, 3, 4), "10", (True,), (1, "4"), -1.5, 64.5, float("nan"), float("inf"), (1, 0), (1, -2), (1, 64.5), (1, float("nan")),
                (1, 4, 0), (1, 4, 17), (1, 4, 2.5), (1, 4, True), None):
        with pytest.raises(ValueError):
            P.check_boundary_weight(bad)


def test_parse_boundary_weight():
    assert P.parse_boundary_weight("10") == (10.0, 4.0, 12) and P.parse_boundary_weight("10,2") == (10.0, 2.0, 6)
    assert P.parse_boundary_weight("0.5,2.5,3") == (0.5, 2.5, 3) and P.parse_boundary_weight("-1") == (-1.0, 4.0, 12)
    assert P.parse_boundary_weight("0") == (0.0, 4.0, 12) and P.parse_boundary_weight("1e1,4e0,16") == (10.0, 4.0, 16)
    for bad in ("", " 10", "10 ", "10,", ",4", "10,4,", "10,4,3,2", "ten", "10,4,3.0", "10,4,x", "65", "-2", "1,0", "1,65", "1,4,0", "1,4,17", "nan", "inf",
                "1, 4"):
        with pytest.raises(ValueError):
            P.parse_boundary_weight(bad)


# ------------------------------------------------------------------------------------------------- command line
def test_cli_good_forms():
    base = ["prog", "a", "b"]
    assert cli.parse_boundary_weight(base) == (base, None)
    assert cli.parse_boundary_weight(base + ["--boundary-weight=10"]) == (base, (10.0, 4.0, 12))
    assert cli.parse_boundary_weight(["prog", "--boundary-weight=5,2", "a", "b"]) == (base, (5.0, 2.0, 6))
    assert cli.parse_boundary_weight(["prog", "a", "--boundary-weight=5,2,9", "b"]) == (base, (5.0, 2.0, 9))
    assert cli.parse_boundary_weight(["prog", "a", "--boundary-weight=0", "b"]) == (base, (0.0, 4.0, 12))


@pytest.mark.parametrize("arg", ["--boundary-weight", "--boundary-weight=", "--boundary-weight=-2", "--boundary-weight=nan", "--boundary-weight=65",
                                 "--boundary-weight=ten", "--boundary-weight=1,0", "--boundary-weight=1,4,17", "--boundary-weight=1,4,2.5",
                                 "--boundary-weight= 2", "--boundary-weight=1,2,3,4"])
def test_cli_bad_forms_name_the_option_and_the_form(arg):
    with pytest.raises(ValueError) as e:
        cli.parse_boundary_weight(["prog", "a", arg])
    msg = str(e.value)
    assert "--boundary-weight=a[,sigma[,R]]" in msg and "[-1, 64]" in msg and "1..16" in msg


def test_cli_twice_is_refused():
    with pytest.raises(ValueError, match="--boundary-weight given more than once"):
        cli.parse_boundary_weight(["prog", "--boundary-weight=2", "x", "--boundary-weight=2"])


def test_cli_beside_the_other_loss_options():
    argv = ["prog", "p1", "--focal-gamma=2", "--boundary-weight=10,3", "--class-weights=median", "p2", "--scale-jitter=0.8,1.2"]
    argv, cw = cli.parse_class_weights(argv, 6)
    argv, g = cli.parse_focal_gamma(argv)
    argv, bw = cli.parse_boundary_weight(argv)
    argv, sj = cli.parse_scale_jitter(argv)
    assert (argv, cw, g, bw, sj) == (["prog", "p1", "p2"], "median", 2.0, (10.0, 3.0, 9), (0.8, 1.2))
    argv0 = ["prog", "--boundary-weight=2", "x"]
    assert cli.parse_focal_gamma(argv0) == (argv0, None) and cli.parse_class_weights(argv0, 6) == (argv0, None)
    assert cli.parse_boundary_scores(argv0) == (argv0, None)            # --boundary-scores is another option and leaves this one alone


def test_cli_main_reports_a_bad_option_in_all_three_flavours():
    for main in (cli.main, cli.main_coffee, cli.main_contest):
        with pytest.raises(SystemExit) as e:
            main(["prog", "--boundary-weight=-2"], device="cpu")
        assert "--boundary-weight" in str(e.value) and "[-1, 64]" in str(e.value)
        with pytest.raises(SystemExit) as e:
            main(["prog", "--boundary-weight=1", "--boundary-weight=2"], device="cpu")
        assert "--boundary-weight given more than once" in str(e.value)
        with pytest.raises(SystemExit) as e:                # a good value is taken out of argv: what is left is too short, the usage line
            main(["prog", "--boundary-weight=10,4,12"], device="cpu")
        assert str(e.value).startswith("Usage: ")


def test_cli_outside_training_is_refused():
    isprs = ["prog"] + ["x"] * 15
    for process in ("validate_test", "generate_final_maps"):
        with pytest.raises(SystemExit) as e:
            cli.main(isprs + [process, "--boundary-weight=2"], device="cpu")
        assert str(e.value) == "--boundary-weight applies to the training process only"
    contest = ["prog", "--boundary-weight=2"] + ["x"] * 13
    with pytest.raises(SystemExit) as e:
        cli.main_contest(contest + ["test"], device="cpu")
    assert "--boundary-weight applies to the train operation only" in str(e.value)


def test_cli_flag_reaches_the_loops(monkeypatch):
    """coffee's main hands the triple to loops_indexed.train (the two other flavours pass it the same way)"""
    import inspect
    from drs_amd import loops_indexed as LI
    for fn in (loops.train, LI.train):
        assert inspect.signature(fn).parameters["boundary_weight"].default is None
    src = inspect.getsource(cli)
    assert src.count("boundary_weight=boundary_weight") == 3


# ------------------------------------------------------------------------------------------------- checkpoint
class _FakeNet(object):
    """what save_checkpoint / load_checkpoint / setup_boundary_weight touch of a net"""

    def __init__(self):
        self._bw, self._g, self._w = None, 0.0, None
        self.state = {"conv1/weights": np.arange(6, dtype=np.float32), "main_global_step": np.array(0, dtype=np.int64)}

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, d):
        self.state = {k: np.asarray(v) for k, v in d.items()}

    def set_class_weights(self, w):
        self._w = None if w is None else P.check_class_weights(w, 4)

    @property
    def class_weights(self):
        return None if self._w is None else self._w.copy()

    def set_focal_gamma(self, g):
        self._g = 0.0 if g is None else P.check_focal_gamma(g)

    @property
    def focal_gamma(self):
        return self._g

    def set_boundary_weight(self, bw):
        self._bw = None if bw is None else P.check_boundary_weight(bw)

    @property
    def boundary_weight(self):
        return None if self._bw is None or self._bw[0] == 0.0 else self._bw


def test_checkpoint_round_trip_of_the_triple(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet()
    a.set_boundary_weight((0.1, 2.5, 7))
    loops.save_checkpoint(a, out, 1000, np.zeros(3, np.float32), np.ones(3, np.int32), np.zeros(3, np.int32))
    assert os.path.isfile(out + "boundary_weight_step_1000.npy") and os.path.isfile(out + "patch_occur_step_1000.npy")
    assert not os.path.exists(out + "focal_gamma_step_1000.npy") and not os.path.exists(out + "class_weights_step_1000.npy")
    side = np.load(out + "boundary_weight_step_1000.npy")
    assert side.dtype == np.float64 and side.tolist() == [0.1, 2.5, 7.0]
    with np.load(out + "model-1000.npz") as d:
        assert sorted(d.files) == sorted(a.state)            # the model file keeps the TensorFlow variable set
    b = _FakeNet()
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-1000")
    text = capsys.readouterr().out
    assert "Boundary weight (restored from " + out + "boundary_weight_step_1000.npy): a 0.1 sigma 2.5 R 7" in text
    assert b.boundary_weight == a.boundary_weight == (0.1, 2.5, 7)          # the same doubles: the same loss
    # beside the two other side files
    a.set_focal_gamma(2)
    a.set_class_weights([1, 2, 3, 4])
    loops.save_checkpoint(a, out, 1001)
    c = _FakeNet()
    loops.load_checkpoint(c, out + "model-1001.npz")
    assert c.boundary_weight == a.boundary_weight and c.focal_gamma == 2.0 and c.class_weights.tobytes() == a.class_weights.tobytes()


def test_checkpoint_without_the_option_leaves_none(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet()
    loops.save_checkpoint(a, out, 7)
    a.set_boundary_weight((0, 4, 12))
    loops.save_checkpoint(a, out, 7)
    assert not os.path.exists(out + "boundary_weight_step_7.npy")            # a = 0 is unset
    b = _FakeNet()
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-7")
    assert b.boundary_weight is None and "Boundary weight" not in capsys.readouterr().out
    a.set_boundary_weight(5)
    loops.save_checkpoint(a, out, 8)
    loops.load_checkpoint(b, out + "model-7")                                # another step's triple is not picked up
    assert b.boundary_weight is None


def test_setup_boundary_weight_overrides_and_says_so():
    from drs_amd.net import NoComm
    lines = []
    net = _FakeNet()
    assert loops.setup_boundary_weight(net, 0, NoComm(), lines.append) == (0.0, 4.0, 12) and lines == [] and net.boundary_weight is None
    assert loops.setup_boundary_weight(net, (10, 4), NoComm(), lines.append) == (10.0, 4.0, 12) and net.boundary_weight == (10.0, 4.0, 12)
    assert len(lines) == 1 and "Boundary weight: a 10 sigma 4 R 12" in lines[0] and "replacing" not in lines[0]
    loops.setup_boundary_weight(net, (2, 1.5, 3), NoComm(), lines.append)
    assert len(lines) == 2 and "a 2 sigma 1.5 R 3" in lines[1] and "replacing the triple restored from the checkpoint, a 10 sigma 4 R 12" in lines[1]
    loops.setup_boundary_weight(net, 0, NoComm(), lines.append)
    assert net.boundary_weight is None and len(lines) == 3 and "a 0 (off" in lines[2] and "replacing" in lines[2]
    with pytest.raises(ValueError):
        loops.setup_boundary_weight(net, 65, NoComm(), lines.append)

    class TwoRanks(NoComm):
        def agree(self, values, what):
            self.seen = (list(values), what)
    comm = TwoRanks()
    loops.setup_boundary_weight(net, (10, 4, 12), comm, lines.append)
    bits = np.asarray([10.0, 4.0], dtype=np.float64).view(np.uint32).tolist()
    assert comm.seen == (bits + [12], "boundary weight")                    # every rank is held to the same triple, on its bits


# ------------------------------------------------------------------------------------------------- header, signatures, exports
def test_header_lib_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    new = ("drs_patch_boundary_weight", "drs_classifier_loss_pixel", "drs_net_set_boundary_weight", "drs_net_get_boundary_weight")
    exported = set(re.findall(r" T (drs_[a-z0-9_]+)$", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                                                                        check=True).stdout, flags=re.M))
    lib = _lib.load()
    for name in new:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", hdr, flags=re.M)
        assert m, name
        nargs = len([a for a in m.group(1).replace("\n", " ").split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, (name, nargs)
        assert name in exported and hasattr(lib, name)
    # the two op-level entry points sit in a section of their own after the step level, as the component entry points do
    step = hdr.index("Step level: the reference's three `sess.run` call shapes")
    assert hdr.index("int drs_patch_boundary_weight(") > hdr.index("int drs_component_census(") > step
    assert hdr.index("int drs_classifier_loss_pixel(") > step and step < hdr.index("int drs_net_set_boundary_weight(") < hdr.index("Whole-map level")
    # the pixel form is the focal form plus one pointer
    focal, pixel = _lib.SIGNATURES["drs_classifier_loss_focal"][1], _lib.SIGNATURES["drs_classifier_loss_pixel"][1]
    assert pixel[:16] == focal[:16] and pixel[17:] == focal[16:] and pixel[16] is C.c_void_p
