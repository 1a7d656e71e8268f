"""Host side of online hard example mining in the training loss: the numpy statement (tests/hard_mining_ref.py) -- the
kept count at its edges, nested kept sets, shard invariance, its gradient against fp64 autograd and central finite differences --
the argument domains of the new entry point and of the setter, the bound buffer, the command-line option, the checkpoint side file,
and the agreement of include/drs.h, _lib.py and the library's exports.  No GPU: the kernel and the step are held by
tests/test_gpu_hard_mining.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from drs_amd import _lib, cli, loops, patches as P

import hard_mining_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the reference
def _case(seed=0, B=3, n=41, K=4):
    """patch 0: every pixel in the loss; patch 1: a few labels >= K, a loss mask with holes; patch 2: no pixel in the loss"""
    rng = np.random.default_rng(seed)
    lg = rng.normal(size=(B, n, K)) * 2.0
    y = rng.integers(0, K, size=(B, n))
    y[1, :3] = (K, 200, 255)
    lm = (rng.random((B, n)) < 0.8).astype(np.uint8)
    lm[0] = 1
    lm[2] = 0
    return lg, y, lm


def test_kept_count_at_its_edges():
    kc = HR.kept_count
    assert kc(4096, 0.25, 0) == 1024 and kc(4096, 0.5, 0) == 2048                 # keep n_b integral: no pixel more
    assert kc(4097, 0.25, 0) == 1025 and kc(10, 0.11, 0) == 2                     # otherwise the ceiling
    assert kc(4096, 1.0 / 4096, 0) == 1 and kc(289, 1.0 / 4096, 0) == 1 and kc(1, 1e-300, 0) == 1   # keep tiny: one pixel, never none
    assert kc(289, 0.25, 300) == 289 and kc(5, 0.5, 1 << 23) == 5                 # min_keep > n_b: everything
    assert kc(289, 0.25, 100) == 100 and kc(289, 0.5, 100) == 145                 # min_keep is a floor
    assert kc(0, 0.25, 0) == 0 and kc(0, 0.25, 300) == 0 and kc(0, 1.0, 0) == 0   # nothing in the loss: nothing kept
    assert kc(289, 1.0, 0) == 289 and kc((1 << 24) - 1, 1.0, 0) == (1 << 24) - 1
    for n in (1, 7, 289, 4096, 4225):                                             # 1 <= k_b <= n_b for every n_b >= 1
        for keep in (1e-9, 1.0 / 4096, 0.1, 0.25, 1.0 / 3, 0.5, 0.999, 1.0):
            for mk in (0, 1, 300):
                k = kc(n, keep, mk)
                assert 1 <= k <= n and k >= min(n, mk) and k >= keep * n - 1e-9 and (k == n or k < max(keep * n + 1, mk + 1))


def test_reference_selection_ties_empty_patch_and_scale():
    lg, y, lm = _case()
    r = HR.mined(lg, y, 4, 0.25, 0, loss_mask=lm)
    assert r["n"].tolist() == [41, int(r["inl"][1].sum()), 0] and r["k"][0] == 11 and r["k"][2] == 0
    assert not r["inl"][1, :3].any() and r["kept"].sum(axis=1).tolist() == r["k"].tolist()
    assert not r["kept"][~r["inl"]].any() and not r["weight"][2].any() and not r["grad"][2].any()
    for b in (0, 1):          # every kept key >= every in-loss key left out; the weights are n_b / k_b in fp32, 0 elsewhere
        out = r["inl"][b] & ~r["kept"][b]
        assert r["ce"][b][r["kept"][b]].min() >= r["ce"][b][out].max()
        assert (r["weight"][b][r["kept"][b]] == np.float32(r["n"][b] / r["k"][b])).all() and not r["weight"][b][~r["kept"][b]].any()
    # each patch contributes the mean of its kept terms, counted by its share of the in-loss pixels
    want = sum(r["n"][b] * r["ce"][b][r["kept"][b]].mean() for b in (0, 1)) / r["inl"].sum()
    assert abs(r["loss"] - want) < 1e-6 * want                                 # (fp32 scale: 2^-24 relative)
    # all keys equal: only the tie rule decides -- the lowest indices in the loss
    keys = np.full((1, 20), 0.75, dtype=np.float32)
    inl = np.ones((1, 20), dtype=bool)
    inl[0, 2] = False
    kept, nb, kb = HR.select(keys, inl, 0.25, 0)
    assert nb[0] == 19 and kb[0] == 5 and np.flatnonzero(kept[0]).tolist() == [0, 1, 3, 4, 5]
    # k_b = n_b: scale exactly 1, an incoming map leaves as it came
    w_in = np.random.default_rng(1).random((1, 20)).astype(np.float32)
    w, kb = HR.weights(keys, inl, 1.0, 0, w_in)
    assert kb[0] == 19 and (w[inl] == w_in[inl]).all() and not w[~inl].any()
    w, _ = HR.weights(keys, inl, 0.25, 0, w_in)
    assert (w[kept] == np.float32(19 / 5) * w_in[kept]).all() and w.dtype == np.float32


def test_kept_sets_are_nested_as_keep_grows():
    lg, y, lm = _case(seed=2, n=97)
    prev = None
    for keep in (1.0 / 4096, 0.1, 0.25, 0.5, 0.75, 1.0):
        for min_keep in (0, 30):
            kept = HR.mined(lg, y, 4, keep, min_keep, loss_mask=lm)["kept"]
            if min_keep == 0:
                assert prev is None or not (prev & ~kept).any()
                prev = kept
            else:
                assert not (HR.mined(lg, y, 4, keep, 0, loss_mask=lm)["kept"] & ~kept).any()       # a floor only adds
    assert (prev == HR.in_loss(y, 4, lm)).all()                                                     # keep = 1: everything in the loss


def test_shard_invariance_in_the_reference():
    """the kept set, the weights, the loss and the gradient of B = 4 are those of its two halves, each with the global inv_n: what lets
    a sharded batch train as the whole one does with no collective"""
    K = 3
    rng = np.random.default_rng(3)
    lg = rng.normal(size=(4, 31, K))
    y = rng.integers(0, K + 1, size=(4, 31))            # (a few labels == K: outside the loss)
    lm = (rng.random((4, 31)) < 0.7).astype(np.uint8)
    inv_n = 1.0 / float(HR.in_loss(y, K, lm).sum())
    whole = HR.mined(lg, y, K, 0.3, 5, lm, inv_n)
    halves = [HR.mined(lg[s], y[s], K, 0.3, 5, lm[s], inv_n) for s in (slice(0, 2), slice(2, 4))]
    for name in ("kept", "weight", "grad", "k"):
        np.testing.assert_array_equal(whole[name], np.concatenate([h[name] for h in halves]))
    assert abs(whole["loss"] - (halves[0]["loss"] + halves[1]["loss"])) < 1e-15


def _gap_to_threshold(r):
    """per patch: the smallest distance of another in-loss key to the threshold key (the smallest kept one)"""
    gaps = []
    for b in range(r["ce"].shape[0]):
        if r["k"][b] == 0 or r["k"][b] == r["n"][b]:
            continue
        keys = np.sort(r["ce"][b][r["inl"][b]])[::-1]
        t = keys[r["k"][b] - 1]
        gaps.append(min(keys[r["k"][b] - 2] - t if r["k"][b] > 1 else np.inf, t - keys[r["k"][b]]))
    return min(gaps)


def test_gradient_against_autograd_and_finite_differences():
    K = 4
    for seed in range(40):                              # a point where no two keys of a patch are within 1e-3 of the threshold key
        lg, y, lm = _case(seed=seed)
        r = HR.mined(lg, y, K, 0.25, 0, loss_mask=lm, inv_n=1.0 / 57.0)
        if _gap_to_threshold(r) > 1e-3:
            break
    assert _gap_to_threshold(r) > 1e-3
    # torch-CPU fp64 autograd of sum w CE with w detached
    t = torch.tensor(lg, dtype=torch.float64, requires_grad=True)
    yy = torch.as_tensor(np.minimum(y, K - 1), dtype=torch.long)
    ce = -torch.log_softmax(t, dim=2).gather(2, yy[..., None])[..., 0]
    w = torch.as_tensor(r["weight"].astype(np.float64))
    loss = (w * ce).sum() / 57.0
    loss.backward()
    assert abs(r["loss"] - float(loss.detach())) < 1e-14 * abs(r["loss"]) and r["loss"] > 0
    np.testing.assert_allclose(r["grad"], t.grad.numpy(), rtol=0, atol=1e-15)
    assert np.abs(r["grad"]).max() > 1e-4 and not r["grad"][~r["kept"]].any()
    # central differences of the mined loss itself (the selection re-made at every point: it does not move, by the gap)
    rng = np.random.default_rng(1)
    h = 1e-6
    for _ in range(24):
        b, i, k = rng.integers(0, 2), rng.integers(0, lg.shape[1]), rng.integers(0, K)
        up, dn = lg.copy(), lg.copy()
        up[b, i, k] += h
        dn[b, i, k] -= h
        ru, rd = HR.mined(up, y, K, 0.25, 0, lm, 1.0 / 57.0), HR.mined(dn, y, K, 0.25, 0, lm, 1.0 / 57.0)
        assert (ru["kept"] == r["kept"]).all() and (rd["kept"] == r["kept"]).all()
        assert abs((ru["loss"] - rd["loss"]) / (2 * h) - r["grad"][b, i, k]) < 1e-8, (b, i, k)


# ------------------------------------------------------------------------------------------------- the entry point's checks
OK, ERR_ARG, ERR_HIP = 0, 1, 2
p0, p1, p2, p3, p4, p5, p6 = [0x10000 + 0x1000 * i for i in range(7)]     # dummy device pointers: host code never dereferences them
NAN, INFTY = float("nan"), float("inf")
ROWS = {
    "drs_patch_hard_weight": (
        [("logits", p0), ("ce", p1), ("labels", p2), ("loss_mask", p3), ("B", 3), ("S", 21), ("K", 6), ("keep", 0.25), ("min_keep", 16),
         ("pixel_weight_in", p4), ("weight_out", p5), ("kept_out", p6)],
        [dict(ce=None), dict(labels=None), dict(weight_out=None), dict(B=0), dict(S=0), dict(B=-3), dict(S=-21), dict(B=1 << 12, S=64),
         dict(B=1, S=4096), dict(B=1 << 20, S=1 << 20), dict(K=0), dict(K=9), dict(K=-1), dict(keep=0.0), dict(keep=-0.25),
         dict(keep=1.0000001), dict(keep=2.0), dict(keep=NAN), dict(keep=INFTY), dict(keep=-INFTY), dict(min_keep=-1), dict(min_keep=1 << 24),
         dict(min_keep=-(1 << 31))],
        [dict(logits=None), dict(loss_mask=None), dict(pixel_weight_in=None), dict(pixel_weight_in=p5), dict(kept_out=None), dict(keep=1.0),
         dict(keep=1e-300), dict(keep=1.0 / 4096), dict(min_keep=0), dict(min_keep=(1 << 24) - 1), dict(K=1), dict(K=8), dict(B=1, S=4095),
         dict(B=1, S=1), dict(keep=1.0, min_keep=300)]),
}


def _call(lib, name, args, change=None):
    a = dict(args)
    assert not change or set(change) <= set(a), (name, change)
    a.update(change or {})
    return getattr(lib, name)(*[a[k] for k, _ in args], None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the in-domain rows would launch kernels on dummy pointers: CPU machines only")
def test_abi_rows():
    """in the manner of tests/test_abi_contract.py: the baseline and every in-domain edge pass validation (what comes back is the
    launch's status), every single violation returns exactly DRS_ERR_ARG"""
    lib = _lib.load()
    for name, (args, bad, good) in ROWS.items():
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
        keep, mk = C.c_double(-7), C.c_int(-7)
        get = lambda: (lib.drs_net_get_hard_mining(h, C.byref(keep), C.byref(mk)), (keep.value, mk.value))   # noqa: E731
        assert get() == (OK, (1.0, 0))                                              # never set: off
        for bad in ((0.0, 0), (-0.5, 0), (1.5, 0), (NAN, 0), (INFTY, 0), (0.25, -1), (0.25, 1 << 24), (1.0, -1), (1.0, 1 << 24), (NAN, -1)):
            assert lib.drs_net_set_hard_mining(h, *bad) == ERR_ARG, bad
        assert get() == (OK, (1.0, 0))                                              # a rejected call changes nothing
        for good in ((0.25, 0), (1.0 / 4096, 1), (0.5, (1 << 24) - 1), (1e-300, 300), (1.0, 300), (0.7, 16)):
            assert lib.drs_net_set_hard_mining(h, *good) == OK
            assert get() == (OK, good)
        assert lib.drs_net_set_hard_mining(h, 0.0, 5) == ERR_ARG and get() == (OK, (0.7, 16))      # ... nor when a pair is in use
        assert lib.drs_net_get_hard_mining(h, None, None) == OK
        assert lib.drs_net_set_hard_mining(None, 0.25, 0) == ERR_ARG and lib.drs_net_get_hard_mining(None, None, None) == ERR_ARG
        # the buffer the step writes the keys into: b_max s_max^2 floats; pixel_weight is still the last entry, loss_mask the one before
        name, nb, dt = C.create_string_buffer(64), C.c_size_t(), C.c_int()
        info, names = {}, []
        for i in range(_lib.query("drs_net_num_buffers", h)):
            _lib.call("drs_net_buffer_info", h, i, name, 64, C.byref(nb), C.byref(dt))
            info[name.value.decode()] = (nb.value, dt.value)
            names.append(name.value.decode())
        assert info["hard_ce"] == (4 * 2 * 17 * 17, info["pixel_weight"][1]) and info["pixel_weight"][0] == 4 * 2 * 17 * 17
        assert names[-1] == "pixel_weight" and names[-2] == "loss_mask" and names.count("hard_ce") == 1
        assert names.index("dice_loss") < names.index("hard_ce") < names.index("logits")
    finally:
        lib.drs_net_destroy(h)


def test_timing_kinds_are_unchanged():
    assert _lib.query("drs_net_num_timing_kinds") == 15


# ------------------------------------------------------------------------------------------------- the pair
def test_check_hard_mining():
    assert P.check_hard_mining(0.25) == (0.25, 0) and P.check_hard_mining((0.5,)) == (0.5, 0) and P.check_hard_mining(1) == (1.0, 0)
    assert P.check_hard_mining((0.25, 300)) == (0.25, 300) and P.check_hard_mining([1.0 / 4096, (1 << 24) - 1]) == (1.0 / 4096, (1 << 24) - 1)
    assert P.check_hard_mining((np.float32(0.5), np.int64(7))) == (0.5, 7) and P.check_hard_mining((0.5, 16.0)) == (0.5, 16)
    assert type(P.check_hard_mining((0.5, np.int64(7)))[1]) is int and type(P.check_hard_mining(1)[0]) is float
    for bad in ((), (0.5, 1, 2), "0.5", (True,), (0.5, True), (0.5, "1"), 0, 0.0, -0.5, 1.5, NAN, INFTY, (0.5, -1), (0.5, 1 << 24), (0.5, 1.5),
                (0.5, NAN), (0.5, INFTY), None):
        with pytest.raises(ValueError):
            P.check_hard_mining(bad)


def test_parse_hard_mining():
    assert P.parse_hard_mining("0.25") == (0.25, 0) and P.parse_hard_mining("0.5,300") == (0.5, 300) and P.parse_hard_mining("1") == (1.0, 0)
    assert P.parse_hard_mining("2.5e-1,0") == (0.25, 0) and P.parse_hard_mining("1,16777215") == (1.0, (1 << 24) - 1)
    for bad in ("", " 0.5", "0.5 ", "0.5,", ",3", "0.5,3,4", "half", "0.5,x", "0.5,1.5", "0.5,-1", "0.5,16777216", "0", "-0.5", "1.5", "nan", "inf",
                "0.5, 3", "0.5,+3", "0.5,1e2"):
        with pytest.raises(ValueError):
            P.parse_hard_mining(bad)


# ------------------------------------------------------------------------------------------------- command line
def test_cli_good_forms():
    base = ["prog", "a", "b"]
    assert cli.parse_hard_mining(base) == (base, None)
    assert cli.parse_hard_mining(base + ["--hard-mining=0.25"]) == (base, (0.25, 0))
    assert cli.parse_hard_mining(["prog", "--hard-mining=0.5,300", "a", "b"]) == (base, (0.5, 300))
    assert cli.parse_hard_mining(["prog", "a", "--hard-mining=1", "b"]) == (base, (1.0, 0))


@pytest.mark.parametrize("arg", ["--hard-mining", "--hard-mining=", "--hard-mining=0", "--hard-mining=-1", "--hard-mining=nan", "--hard-mining=1.5",
                                 "--hard-mining=half", "--hard-mining=0.5,", "--hard-mining=0.5,1.5", "--hard-mining=0.5,-3", "--hard-mining= 0.5",
                                 "--hard-mining=0.5,16777216", "--hard-mining=0.5,1,2"])
def test_cli_bad_forms_name_the_option_and_the_form(arg):
    with pytest.raises(ValueError) as e:
        cli.parse_hard_mining(["prog", "a", arg])
    msg = str(e.value)
    assert "--hard-mining=keep[,min_keep]" in msg and "(0, 1]" in msg and "16777215" in msg


def test_cli_twice_is_refused():
    with pytest.raises(ValueError, match="--hard-mining given more than once"):
        cli.parse_hard_mining(["prog", "--hard-mining=0.5", "x", "--hard-mining=0.5"])


def test_cli_beside_the_other_loss_options():
    argv = ["prog", "p1", "--focal-gamma=2", "--hard-mining=0.25,64", "--dice-weight=1,0.3,0.7", "--boundary-weight=10,3", "--class-weights=median", "p2"]
    argv, cw = cli.parse_class_weights(argv, 6)
    argv, g = cli.parse_focal_gamma(argv)
    argv, bw = cli.parse_boundary_weight(argv)
    argv, dc = cli.parse_dice(argv)
    argv, hm = cli.parse_hard_mining(argv)
    assert (argv, cw, g, bw, dc, hm) == (["prog", "p1", "p2"], "median", 2.0, (10.0, 3.0, 9), (1.0, 0.3, 0.7, 1.0), (0.25, 64))
    argv0 = ["prog", "--hard-mining=0.5", "x"]
    assert cli.parse_focal_gamma(argv0) == (argv0, None) and cli.parse_boundary_weight(argv0) == (argv0, None) and cli.parse_dice(argv0) == (argv0, None)
    assert cli.parse_class_weights(argv0, 6) == (argv0, None)


def test_cli_main_reports_a_bad_option_in_all_three_flavours():
    for main in (cli.main, cli.main_coffee, cli.main_contest):
        with pytest.raises(SystemExit) as e:
            main(["prog", "--hard-mining=2"], device="cpu")
        assert "--hard-mining=keep[,min_keep]" in str(e.value) and "(0, 1]" in str(e.value)
        with pytest.raises(SystemExit) as e:
            main(["prog", "--hard-mining=0.5", "--hard-mining=0.25"], device="cpu")
        assert "--hard-mining given more than once" in str(e.value)
        with pytest.raises(SystemExit) as e:                # a good value is taken out of argv: what is left is too short, the usage line
            main(["prog", "--hard-mining=0.25,16"], device="cpu")
        assert str(e.value).startswith("Usage: ")


def test_cli_outside_training_is_refused():
    isprs = ["prog"] + ["x"] * 15
    for process in ("validate_test", "generate_final_maps"):
        with pytest.raises(SystemExit) as e:
            cli.main(isprs + [process, "--hard-mining=0.5"], device="cpu")
        assert str(e.value) == "--hard-mining applies to the training process only"
    contest = ["prog", "--hard-mining=0.5"] + ["x"] * 13
    with pytest.raises(SystemExit) as e:
        cli.main_contest(contest + ["test"], device="cpu")
    assert "--hard-mining applies to the train operation only" in str(e.value)


def test_cli_flag_reaches_the_loops():
    from drs_amd import loops_indexed as LI
    for fn in (loops.train, LI.train):
        assert inspect.signature(fn).parameters["hard_mining"].default is None
        assert "setup_hard_mining(net, hard_mining, comm, say)" in inspect.getsource(fn) and "mined" in fn.__doc__
    assert inspect.getsource(cli).count("hard_mining=hard_mining") == 3
    assert inspect.getsource(cli).count("argv, hard_mining = parse_hard_mining(argv)") == 3
    assert "save_hard_mining(net, output_path, step)" in inspect.getsource(LI.train)


# ------------------------------------------------------------------------------------------------- checkpoint
class _FakeNet(object):
    """what save_checkpoint / load_checkpoint / setup_hard_mining touch of a net"""

    def __init__(self):
        self._h = None
        self.state = {"conv1/weights": np.arange(6, dtype=np.float32), "main_global_step": np.array(0, dtype=np.int64)}

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, d):
        self.state = {k: np.asarray(v) for k, v in d.items()}

    class_weights, focal_gamma, boundary_weight, dice = None, 0.0, None, None

    def set_hard_mining(self, h):
        self._h = None if h is None else P.check_hard_mining(h)

    @property
    def hard_mining(self):
        return None if self._h is None or self._h[0] == 1.0 else self._h


def test_checkpoint_round_trip_of_the_pair(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet()
    a.set_hard_mining((0.1, 300))
    loops.save_checkpoint(a, out, 1000, np.zeros(3, np.float32), np.ones(3, np.int32), np.zeros(3, np.int32))
    assert os.path.isfile(out + "hard_mining_step_1000.npy") and os.path.isfile(out + "patch_occur_step_1000.npy")
    assert not os.path.exists(out + "focal_gamma_step_1000.npy") and not os.path.exists(out + "dice_step_1000.npy")
    side = np.load(out + "hard_mining_step_1000.npy")
    assert side.dtype == np.float64 and side.tolist() == [0.1, 300.0]
    with np.load(out + "model-1000.npz") as d:
        assert sorted(d.files) == sorted(a.state)            # the model file keeps the TensorFlow variable set
    b = _FakeNet()
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-1000")
    text = capsys.readouterr().out
    assert "Hard mining (restored from " + out + "hard_mining_step_1000.npy): keep 0.1 min_keep 300" in text
    assert b.hard_mining == a.hard_mining == (0.1, 300) and type(b.hard_mining[1]) is int      # the same double: the same selection


def test_checkpoint_without_the_option_leaves_none(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _FakeNet()
    loops.save_checkpoint(a, out, 7)
    a.set_hard_mining((1, 300))
    loops.save_checkpoint(a, out, 7)
    assert not os.path.exists(out + "hard_mining_step_7.npy")       # keep = 1 is unset, whatever min_keep is
    b = _FakeNet()
    capsys.readouterr()
    loops.load_checkpoint(b, out + "model-7")
    assert b.hard_mining is None and "Hard mining" not in capsys.readouterr().out
    a.set_hard_mining(0.5)
    loops.save_checkpoint(a, out, 8)
    loops.load_checkpoint(b, out + "model-7")                # another step's pair is not picked up
    assert b.hard_mining is None


def test_setup_hard_mining_overrides_and_says_so():
    from drs_amd.net import NoComm
    lines = []
    net = _FakeNet()
    assert loops.setup_hard_mining(net, 1, NoComm(), lines.append) == (1.0, 0) and lines == [] and net.hard_mining is None
    assert loops.setup_hard_mining(net, (0.25, 16), NoComm(), lines.append) == (0.25, 16) and net.hard_mining == (0.25, 16)
    assert len(lines) == 1 and "Hard mining: keep 0.25 min_keep 16" in lines[0] and "replacing" not in lines[0] and "mined" in lines[0]
    loops.setup_hard_mining(net, 0.5, NoComm(), lines.append)
    assert len(lines) == 2 and "Hard mining: keep 0.5 min_keep 0" in lines[1]
    assert "replacing the pair restored from the checkpoint, keep 0.25 min_keep 16" in lines[1]
    loops.setup_hard_mining(net, 1, NoComm(), lines.append)
    assert net.hard_mining is None and len(lines) == 3 and "keep 1 (off" in lines[2] and "replacing" in lines[2]
    with pytest.raises(ValueError):
        loops.setup_hard_mining(net, 1.5, NoComm(), lines.append)

    class TwoRanks(NoComm):
        def agree(self, values, what):
            self.seen = (list(values), what)
    comm = TwoRanks()
    loops.setup_hard_mining(net, (0.3, 7), comm, lines.append)
    assert comm.seen == (np.asarray([0.3], dtype=np.float64).view(np.uint32).tolist() + [7], "hard mining")


def test_both_nets_carry_the_option_and_say_which_loss_is_printed():
    from drs_amd import engine, net, oplevel
    for cls in (engine.EngineNet, oplevel.OpLevelNet):
        assert isinstance(inspect.getattr_static(cls, "hard_mining"), property) and hasattr(cls, "set_hard_mining")
    assert "MINED" in net.DilatedNet.set_hard_mining.__doc__ and "inspection" in loops.hard_mining_weights.__doc__


# ------------------------------------------------------------------------------------------------- header, signatures, exports
def test_header_lib_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    new = ("drs_patch_hard_weight", "drs_net_set_hard_mining", "drs_net_get_hard_mining")
    exported = set(re.findall(r" T (drs_[a-z0-9_]+)$", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                                                                        check=True).stdout, flags=re.M))
    lib = _lib.load()
    for name in new:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", hdr, flags=re.M)
        assert m, name
        nargs = len([a for a in m.group(1).replace("\n", " ").split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, (name, nargs)
        assert name in exported and hasattr(lib, name)
    # the op-level entry point sits in a section of its own at the end of the header, after the Dice one; the setter beside the Dice setter
    step = hdr.index("Step level: the reference's three `sess.run` call shapes")
    assert hdr.index("int drs_patch_hard_weight(") > hdr.index(" * Training level: hard example mining (opt-in") > hdr.index("int drs_dice_loss_add(") > step
    assert step < hdr.index("int drs_net_get_dice(") < hdr.index("int drs_net_set_hard_mining(") < hdr.index("int drs_net_get_hard_mining(") < hdr.index("Whole-map level")
    sig = _lib.SIGNATURES["drs_patch_hard_weight"][1]
    assert sig[7] is C.c_double and sig[8] is C.c_int and _lib.SIGNATURES["drs_net_set_hard_mining"][1][1:] == [C.c_double, C.c_int]
