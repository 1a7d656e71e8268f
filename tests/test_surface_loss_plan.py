"""Host side of the boundary (surface) loss of the training loss: the numpy statement (tests/surface_loss_ref.py) against
scipy's distance_transform_edt through the published formula, against a brute-force minimum over all pairs, and against fp64 autograd
of sum softmax phi; the clip and the empty cases; the argument domains of the new entry points and of the setter, the new bound
buffers, the option's parsers, the side file, and header = _lib.py = exports.  The kernel itself is held by
tests/test_gpu_surface_loss.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import surface_loss_ref as SR
from drs_amd import _lib, cli, loops
from drs_amd import loops_indexed as LI
from drs_amd import patches as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_HIP = 0, 1, 2
NAN, INFTY = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------- the statement
def _blobs(rng, B, S, K):
    """labels in patches of a few pixels a side: contours, classes of several pixels"""
    c = max(1, S // 4)
    coarse = rng.integers(0, K, size=(B, (S + c - 1) // c, (S + c - 1) // c))
    return np.repeat(np.repeat(coarse, c, axis=1), c, axis=2)[:, :S, :S].astype(np.uint8)


def _brute(y, K, cnt):
    """the signed squared distances by the minimum over all pairs of pixels, O(n^2)"""
    B, S, _ = y.shape
    yy, xx = np.mgrid[0:S, 0:S]
    pos = np.stack([yy.reshape(-1), xx.reshape(-1)], axis=1).astype(np.int64)
    d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(axis=2)
    out = np.zeros((B, S * S, K), dtype=np.int64)
    for b in range(B):
        lab, ok = y[b].reshape(-1), cnt[b].reshape(-1)
        for c in range(K):
            A, O = ok & (lab == c), ok & (lab != c)
            if not A.any() or not O.any():
                continue
            out[b, O, c] = d2[np.ix_(O, A)].min(axis=1)
            out[b, A, c] = -d2[np.ix_(A, O)].min(axis=1)
    return out.reshape(B, S, S, K)


def test_statement_against_scipy_through_the_published_formula():
    """fully counted patches: phi = edt(~pos) ~pos - (edt(pos) - 1) pos, the convention of the paper's code; the difference is 0"""
    from scipy.ndimage import distance_transform_edt as edt
    rng = np.random.default_rng(0)
    for S, K in ((13, 3), (24, 6), (37, 2)):
        for y in (_blobs(rng, 2, S, K), rng.integers(0, K, size=(2, S, S)).astype(np.uint8)):
            phi2 = SR.signed_sq_dist(y, K)
            phi = SR.phi_of(phi2)
            for b in range(y.shape[0]):
                for c in range(K):
                    pos = y[b] == c
                    if not pos.any() or pos.all():
                        assert not phi2[b, :, :, c].any()
                        continue
                    want = edt(~pos) * ~pos - (edt(pos) - 1.0) * pos
                    assert np.array_equal(phi[b, :, :, c], want), (S, K, b, c)
                    assert np.array_equal(np.abs(phi2[b, :, :, c]), np.rint(edt(~pos) ** 2 + edt(pos) ** 2).astype(np.int64))


def test_statement_against_brute_force_with_holes():
    """loss-mask holes, valid holes and labels >= K are never a site and carry no term; distances pass over them"""
    rng = np.random.default_rng(1)
    B, S, K = 3, 15, 4
    y = _blobs(rng, B, S, K)
    y[rng.random(size=y.shape) < 0.1] = K + 1
    lm = (rng.random(size=y.shape) < 0.8).astype(np.uint8)
    va = (rng.random(size=y.shape) < 0.8).astype(np.uint8)
    for loss_mask, valid in ((None, None), (lm, None), (None, va), (lm, va)):
        cnt = SR.counted(y, K, loss_mask, valid)
        got = SR.signed_sq_dist(y, K, loss_mask, valid)
        assert np.array_equal(got, _brute(y, K, cnt))
        assert not got[~cnt].any()
        assert (got[cnt & (y < K)][np.arange(int(cnt.sum())), y[cnt]] <= 0).all()         # inside its own class: never positive
    assert np.array_equal(SR.counted(y, K, lm, va), (y < K) & (lm != 0) & (va != 0))


def test_known_answers():
    y = np.zeros((1, 5, 5), dtype=np.uint8)
    y[0, 2, 2] = 1                                                   # one pixel of class 1 in the middle
    phi2 = SR.signed_sq_dist(y, 2)
    yy, xx = np.mgrid[0:5, 0:5]
    d2 = (yy - 2) ** 2 + (xx - 2) ** 2
    assert np.array_equal(phi2[0, :, :, 1], np.where(d2 == 0, -1, d2))
    assert np.array_equal(phi2[0, :, :, 0], np.where(d2 == 0, 1, -d2))
    phi = SR.phi_of(phi2)
    assert phi[0, 2, 2, 1] == 0.0 and not np.signbit(phi[0, 2, 2, 1])          # 1 - sqrt(1): exactly +0 on the contour's inner side
    assert phi[0, 0, 0, 1] == np.sqrt(8.0) and phi[0, 0, 0, 0] == 1.0 - np.sqrt(8.0)
    g64, g32 = SR.grad_map(phi2, 2.5)
    assert g32.dtype == np.float32 and g32[0, 0, 0, 1] == np.float32(2.5 * np.sqrt(8.0)) and not np.signbit(g32[0, 2, 2, 1])


def test_clip():
    rng = np.random.default_rng(2)
    y = _blobs(rng, 2, 21, 3)
    phi2 = SR.signed_sq_dist(y, 3)
    phi = SR.phi_of(phi2)
    assert phi.max() > 3.0 and phi.min() < -3.0
    g64, g32 = SR.grad_map(phi2, 0.5, 3.0)
    assert np.array_equal(g64, 0.5 * np.clip(phi, -3.0, 3.0)) and g64.max() == 1.5 and g64.min() == -1.5
    assert np.array_equal(SR.grad_map(phi2, 0.5, 0.0)[0], 0.5 * phi)          # clip 0: none
    assert np.array_equal(SR.grad_map(phi2, 0.5, 32768.0)[0], 0.5 * phi)


def test_empty_cases_give_zeros():
    rng = np.random.default_rng(3)
    S, K = 9, 3
    y = rng.integers(0, 2, size=(3, S, S)).astype(np.uint8)          # class 2 absent everywhere
    y[1] = 1                                                         # patch 1: one class fills it
    lm = np.ones_like(y)
    lm[2] = 0                                                        # patch 2: nothing counted
    lg = rng.normal(size=(3, S, S, K)) * 3
    out = SR.surface_loss(lg, y, K, 1.5, loss_mask=lm)
    assert not out["phi2"][..., 2].any() and not out["phi2"][1].any() and not out["phi2"][2].any()
    assert out["phi2"][0, :, :, :2].any()
    assert out["patch_loss"][1] == 0.0 and out["patch_loss"][2] == 0.0 and out["patch_loss"][0] != 0.0
    assert not out["grad"][1].any() and not out["grad"][2].any()
    assert not np.signbit(out["g32"]).any() or (out["g32"][np.signbit(out["g32"])] < 0).all()      # zeros are +0


def test_gradient_against_autograd():
    """dL / dlogit_k = inv_n P_k (g_k - sum_c P_c g_c): fp64 autograd of inv_n sum softmax g over the counted pixels"""
    rng = np.random.default_rng(4)
    B, S, K = 2, 11, 5
    y = _blobs(rng, B, S, K)
    y[rng.random(size=y.shape) < 0.05] = K
    lm = (rng.random(size=y.shape) < 0.8).astype(np.uint8)
    va = (rng.random(size=y.shape) < 0.9).astype(np.uint8)
    lg = rng.normal(size=(B, S, S, K)) * 3
    for clip in (0.0, 2.5):
        out = SR.surface_loss(lg, y, K, 0.75, clip, loss_mask=lm, valid=va, inv_n=1.0 / 777)
        t = torch.tensor(lg, dtype=torch.float64, requires_grad=True)
        g = torch.tensor(out["g32"].astype(np.float64)) * torch.tensor(out["counted"][..., None].astype(np.float64))
        loss = (torch.softmax(t, dim=-1) * g).sum() / 777
        loss.backward()
        assert abs(float(loss.detach()) - out["loss"]) <= 1e-12 * max(1.0, abs(out["loss"]))
        assert np.abs(t.grad.numpy() - out["grad"]).max() <= 1e-14
        assert np.abs(out["grad"]).max() > 1e-5


def test_shard_invariance():
    """everything is per patch: the halves of a batch give the whole batch's maps and terms"""
    rng = np.random.default_rng(5)
    y = _blobs(rng, 4, 12, 3)
    lg = rng.normal(size=(4, 12, 12, 3))
    whole = SR.surface_loss(lg, y, 3, 1.0, inv_n=1e-3)
    for sl in (slice(0, 2), slice(2, 4)):
        part = SR.surface_loss(lg[sl], y[sl], 3, 1.0, inv_n=1e-3)
        assert np.array_equal(part["phi2"], whole["phi2"][sl]) and np.array_equal(part["patch_loss"], whole["patch_loss"][sl])
        assert np.array_equal(part["grad"], whole["grad"][sl])


# ------------------------------------------------------------------------------------------------- the entry points' domains
p0, p1, p2, p3, p4, p5, p6, p7, p8 = (0x10000 * (i + 1) for i in range(9))
BIG = 1 << 40
ROWS = {
    "drs_patch_surface_loss": (
        [("logits", p0), ("labels", p1), ("loss_mask", p2), ("valid", p3), ("B", 3), ("S", 21), ("K", 6), ("lam", 1.5), ("clip", 0.0),
         ("dice_coef", None), ("accumulate", 0), ("phi2_out", p5), ("grad_io", p6), ("patch_loss_out", p7), ("scratch", p8),
         ("scratch_bytes", BIG)],
        [dict(labels=None), dict(grad_io=None), dict(patch_loss_out=None), dict(B=0), dict(S=0), dict(B=-3), dict(S=-21),
         dict(B=1 << 12, S=64), dict(B=1, S=4096), dict(B=1 << 20, S=1 << 20), dict(K=0), dict(K=9), dict(K=-1), dict(lam=0.0),
         dict(lam=-1.0), dict(lam=64.0000001), dict(lam=NAN), dict(lam=INFTY), dict(lam=-INFTY), dict(clip=0.5), dict(clip=-1.0),
         dict(clip=32768.5), dict(clip=NAN), dict(clip=INFTY), dict(scratch=None), dict(scratch_bytes=0), dict(scratch_bytes=3 * 6 * 8 - 1),
         dict(S=129, scratch_bytes=3 * 6 * 8 + 3 * 6 * 66576 - 1), dict(dice_coef=p4, accumulate=1), dict(dice_coef=p4 + 4),
         dict(scratch=p8 + 4), dict(grad_io=p6 + 2), dict(phi2_out=p5 + 2), dict(logits=p0 + 2), dict(patch_loss_out=p7 + 4)],
        [dict(logits=None), dict(loss_mask=None), dict(valid=None), dict(dice_coef=p4), dict(accumulate=1), dict(accumulate=7),
         dict(phi2_out=None), dict(lam=64.0), dict(lam=1e-300), dict(clip=1.0), dict(clip=32768.0), dict(K=1), dict(K=8),
         dict(B=1, S=4095), dict(B=1, S=1), dict(scratch_bytes=3 * 6 * 8), dict(S=129, scratch_bytes=3 * 6 * 8 + 3 * 6 * 66576)]),
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


def test_scratch_bytes():
    q = lambda *a: _lib.query("drs_surface_loss_scratch_bytes", *a)      # noqa: E731
    assert q(3, 21, 6) == 3 * 6 * 8 and q(1, 1, 1) == 16 and q(128, 64, 6) == 128 * 6 * 8 and q(1, 13, 3) == 32
    assert q(1, 128, 2) == 16 and q(1, 129, 2) == 16 + 2 * 66576            # the LDS form up to S = 128; 4 * 129^2 = 66564 -> 66576
    assert q(2, 130, 8) == 2 * 8 * 8 + 2 * 8 * 4 * 130 * 130
    for bad in ((0, 4, 2), (1, 0, 2), (1, 4, 0), (1, 4, 9), (1, 4096, 2), (-1, 4, 2)):
        assert q(*bad) == 0
    for b, s, k in ((1, 50, 2), (4, 128, 6), (4, 129, 6), (2, 300, 8), (1, 1, 1)):     # monotone: a net's scratch, sized at (b_max, s_max), serves every step
        assert q(b, s, k) <= q(b + 1, s, k) and q(b, s, k) <= q(b, s + 1, k) and q(b, s, k) % 16 == 0
        if k < 8:
            assert q(b, s, k) <= q(b, s, k + 1)


def test_setter_domain_getter_and_buffers():
    lib = _lib.load()
    h = C.c_void_p()
    _lib.call("drs_net_create", b"dilated_grsl", 5, 6, 0.005, 2, 17, 0, 0.5, C.byref(h))
    try:
        lam, clip = C.c_double(-7), C.c_double(-7)
        get = lambda: (lib.drs_net_get_surface_loss(h, C.byref(lam), C.byref(clip)), lam.value, clip.value)   # noqa: E731
        assert get() == (OK, 0.0, 0.0)                                                # never set: off
        for bad in ((-0.5, 0.0), (-1e-300, 0.0), (64.0000001, 0.0), (100.0, 4.0), (NAN, 0.0), (INFTY, 0.0), (-INFTY, 0.0), (1.0, 0.5),
                    (1.0, -1.0), (1.0, 32768.5), (1.0, NAN), (1.0, INFTY), (0.0, 0.999), (NAN, NAN)):
            assert lib.drs_net_set_surface_loss(h, *bad) == ERR_ARG, bad
        assert get() == (OK, 0.0, 0.0)                                                # a rejected call changes nothing
        for good in ((1.5, 0.0), (64.0, 32768.0), (1e-300, 1.0), (0.0, 0.0), (0.0, 8.0), (0.25, 20.0)):
            assert lib.drs_net_set_surface_loss(h, *good) == OK
            assert get() == (OK,) + good
        assert lib.drs_net_set_surface_loss(h, NAN, 20.0) == ERR_ARG and lib.drs_net_set_surface_loss(h, 0.5, 0.1) == ERR_ARG
        assert get() == (OK, 0.25, 20.0)                                              # ... nor when a pair is in use
        assert lib.drs_net_get_surface_loss(h, None, None) == OK and lib.drs_net_get_surface_loss(h, C.byref(lam), None) == OK
        assert lib.drs_net_set_surface_loss(None, 1.0, 0.0) == ERR_ARG and lib.drs_net_get_surface_loss(None, None, None) == ERR_ARG
        name, nb, dt = C.create_string_buffer(64), C.c_size_t(), C.c_int()
        info, names = {}, []
        for i in range(_lib.query("drs_net_num_buffers", h)):
            _lib.call("drs_net_buffer_info", h, i, name, 64, C.byref(nb), C.byref(dt))
            info[name.value.decode()] = (nb.value, dt.value)
            names.append(name.value.decode())
        B, K = 2, 6
        f64 = info["dice_loss"][1]
        assert info["surface_loss"] == (8 * B, f64)
        assert info["surface_scratch"] == (_lib.query("drs_surface_loss_scratch_bytes", B, 17, K), f64)
        assert names.count("surface_loss") == 1 and names.count("surface_scratch") == 1 and names.count("region_grad") == 1
        assert names[-1] == "pixel_weight" and names[-2] == "loss_mask"
    finally:
        lib.drs_net_destroy(h)
    assert _lib.query("drs_net_num_timing_kinds") == 15                               # accounted under "classifier_loss": no new kind


# ------------------------------------------------------------------------------------------------- the option
def test_check_surface_loss():
    assert P.check_surface_loss(1.5) == (1.5, 0.0) and P.check_surface_loss((2,)) == (2.0, 0.0) and P.check_surface_loss(0) == (0.0, 0.0)
    assert P.check_surface_loss([64, 32768]) == (64.0, 32768.0) and P.check_surface_loss((0.5, 1)) == (0.5, 1.0)
    assert P.check_surface_loss((np.float32(0.5), np.int64(3))) == (0.5, 3.0)
    assert all(type(v) is float for v in P.check_surface_loss((np.int64(3), np.float32(2))))
    assert P.check_surface_loss((0, 5)) == (0.0, 5.0)                                   # off, the clip kept
    for bad in (-0.1, 64.5, NAN, INFTY, "1", None, True, (1, 2, 3), (), [np.bool_(1)], 1 + 2j, (1, 0.5), (1, -2), (1, 32769), (1, NAN),
                (1, INFTY), (1, "2"), (1, None), (1, True)):
        with pytest.raises(ValueError):
            P.check_surface_loss(bad)


def test_parse_surface_loss():
    assert P.parse_surface_loss("1.5") == (1.5, 0.0) and P.parse_surface_loss("0") == (0.0, 0.0)
    assert P.parse_surface_loss("2.5e-1,20") == (0.25, 20.0) and P.parse_surface_loss("64,32768") == (64.0, 32768.0)
    assert P.parse_surface_loss("1,0") == (1.0, 0.0) and P.parse_surface_loss("1,1.5") == (1.0, 1.5)
    for bad in ("", " 1", "1 ", "1,2,3", "x", "65", "-1", "nan", "inf", "1,", ",1", "1, 2", "1,0.5", "1,x", "1,40000", "1,nan"):
        with pytest.raises(ValueError):
            P.parse_surface_loss(bad)


def test_cli_flag():
    base = ["prog", "a", "b"]
    assert cli.parse_surface_loss(base) == (base, None)
    assert cli.parse_surface_loss(base + ["--surface-loss=1.5"]) == (base, (1.5, 0.0))
    assert cli.parse_surface_loss(["prog", "--surface-loss=0.5,20", "a", "b"]) == (base, (0.5, 20.0))
    assert cli.parse_surface_loss(["prog", "a", "--surface-loss=0", "b"]) == (base, (0.0, 0.0))
    for arg in ("--surface-loss", "--surface-loss=", "--surface-loss=65", "--surface-loss=1,2,3", "--surface-loss=x", "--surface-loss=1,0.5"):
        with pytest.raises(ValueError, match=r"expected --surface-loss=lam\[,clip\]"):
            cli.parse_surface_loss(["prog", "a", arg])
    with pytest.raises(ValueError, match="more than once"):
        cli.parse_surface_loss(["prog", "--surface-loss=0.5", "x", "--surface-loss=0.5"])
    for fn in (loops.train, LI.train):
        assert inspect.signature(fn).parameters["surface_loss"].default is None
        assert "setup_surface_loss(net, surface_loss, comm, say)" in inspect.getsource(fn) and "surface" in fn.__doc__
    assert inspect.getsource(cli).count("surface_loss=surface_loss") == 3
    assert inspect.getsource(cli).count("argv, surface_loss = parse_surface_loss(argv)") == 3
    assert "save_surface_loss(net, output_path, step)" in inspect.getsource(LI.train)
    assert "--surface-loss=lam[,clip]" in cli.__doc__


def test_cli_outside_training_is_refused():
    isprs = ["prog"] + ["x"] * 15
    for process in ("validate_test", "generate_final_maps"):
        with pytest.raises(SystemExit) as e:
            cli.main(isprs + [process, "--surface-loss=2"], device="cpu")
        assert str(e.value) == "--surface-loss applies to the training process only"
    contest = ["prog", "--surface-loss=2,8"] + ["x"] * 13
    with pytest.raises(SystemExit) as e:
        cli.main_contest(contest + ["test"], device="cpu")
    assert "--surface-loss applies to the train operation only" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(isprs + ["training", "--surface-loss=2,0.5"], device="cpu")
    assert "expected --surface-loss=lam[,clip]" in str(e.value)


class _Net(object):
    """what save_checkpoint / load_checkpoint / setup_surface_loss touch of a net"""

    def __init__(self):
        self._s = None

    def state_dict(self):
        return {"w": np.zeros(2, dtype=np.float32)}

    def load_state_dict(self, d):
        pass

    def set_surface_loss(self, v):
        self._s = None if v is None else P.check_surface_loss(v)

    @property
    def surface_loss(self):
        return None if self._s is None or self._s[0] == 0.0 else self._s


def test_side_file_round_trip(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _Net()
    a.set_surface_loss((0.1, 20))
    loops.save_checkpoint(a, out, 1000)
    assert os.path.isfile(out + "surface_loss_step_1000.npy")
    side = np.load(out + "surface_loss_step_1000.npy")
    assert side.dtype == np.float64 and side.tolist() == [0.1, 20.0]
    b = _Net()
    loops.load_checkpoint(b, out + "model-1000")
    assert "Surface loss (restored from " + out + "surface_loss_step_1000.npy): lambda 0.1 clip 20" in capsys.readouterr().out
    assert b.surface_loss == a.surface_loss == (0.1, 20.0)
    a.set_surface_loss(0)
    loops.save_checkpoint(a, out, 7)
    assert not os.path.exists(out + "surface_loss_step_7.npy")             # lam = 0 is unset
    b = _Net()
    loops.load_checkpoint(b, out + "model-7")
    assert b.surface_loss is None and "Surface" not in capsys.readouterr().out


def test_setup_surface_loss_overrides_and_says_so():
    from drs_amd.net import NoComm
    net, lines = _Net(), []
    assert loops.setup_surface_loss(net, 0, NoComm(), lines.append) == (0.0, 0.0) and lines == [] and net.surface_loss is None
    assert loops.setup_surface_loss(net, 1.5, NoComm(), lines.append) == (1.5, 0.0) and net.surface_loss == (1.5, 0.0)
    assert len(lines) == 1 and lines[0].startswith("Surface loss: lambda 1.5 clip none") and "replacing" not in lines[0]
    loops.setup_surface_loss(net, (0.5, 20), NoComm(), lines.append)
    assert net.surface_loss == (0.5, 20.0) and lines[1].startswith("Surface loss: lambda 0.5 clip 20")
    assert "replacing the pair restored from the checkpoint, lambda 1.5 clip none" in lines[1]
    loops.setup_surface_loss(net, 0, NoComm(), lines.append)
    assert net.surface_loss is None and len(lines) == 3 and "lambda 0 (off" in lines[2] and "replacing" in lines[2]
    with pytest.raises(ValueError):
        loops.setup_surface_loss(net, 65, NoComm(), lines.append)

    class TwoRanks(NoComm):
        def agree(self, values, what):
            self.seen = (list(values), what)
    comm = TwoRanks()
    loops.setup_surface_loss(net, (0.3, 7), comm, lines.append)
    assert comm.seen == (np.asarray([0.3, 7.0], dtype=np.float64).view(np.uint32).tolist(), "surface loss")


def test_both_nets_carry_the_option():
    from drs_amd import engine, net, oplevel
    for cls in (engine.EngineNet, oplevel.OpLevelNet, net.DilatedNet):
        assert isinstance(inspect.getattr_static(cls, "surface_loss"), property) and hasattr(cls, "set_surface_loss")
    assert "not mined" in net.DilatedNet.set_surface_loss.__doc__ and "inspection" in loops.surface_loss_grad.__doc__
    src = inspect.getsource(oplevel.OpLevelNet)
    assert src.index('"drs_patch_lovasz_grad"') < src.index('"drs_patch_surface_loss"') < src.index('"drs_classifier_loss_region" if region')


# ------------------------------------------------------------------------------------------------- header, signatures, exports
def test_header_lib_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    new = ("drs_surface_loss_scratch_bytes", "drs_patch_surface_loss", "drs_net_set_surface_loss", "drs_net_get_surface_loss")
    exported = set(re.findall(r" T (drs_[a-z0-9_]+)$", subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                                                                        check=True).stdout, flags=re.M))
    lib = _lib.load()
    for name in new:
        m = re.search(r"^(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\);", hdr, flags=re.M)
        assert m, name
        nargs = len([a for a in m.group(1).replace("\n", " ").split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, (name, nargs)
        assert name in exported and hasattr(lib, name)
    declared = set(re.findall(r"^[a-z_ ]+?\**\s*(drs_[a-z0-9_]+)\s*\(", hdr, flags=re.M))
    assert declared == exported == set(_lib.SIGNATURES), (declared ^ exported, exported ^ set(_lib.SIGNATURES))
    step = hdr.index("Step level: the reference's three `sess.run` call shapes")
    assert hdr.index("int drs_patch_surface_loss(") > hdr.index(" * Training level: boundary (surface) loss (opt-in") > hdr.index("int drs_classifier_loss_region(") > step
    assert step < hdr.index("int drs_net_get_lovasz(") < hdr.index("int drs_net_set_surface_loss(") < hdr.index("int drs_net_get_surface_loss(") < hdr.index("Whole-map level")
    sig = _lib.SIGNATURES["drs_patch_surface_loss"][1]
    assert sig[7] is C.c_double and sig[8] is C.c_double and sig[10] is C.c_int and sig[15] is C.c_size_t
    assert _lib.SIGNATURES["drs_net_set_surface_loss"][1][1:] == [C.c_double, C.c_double]
    assert _lib.SIGNATURES["drs_surface_loss_scratch_bytes"][0] is C.c_size_t
    build = open(os.path.join(ROOT, "dynamic-rs-segmentation_amd", "csrc", "build.sh")).read()
    assert " surface_loss " in re.search(r'^SRCS="([^"]*)"', build, flags=re.M).group(1)
