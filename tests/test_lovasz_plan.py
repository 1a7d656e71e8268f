"""Host side of the Lovasz-softmax term of the training loss: the numpy statement (tests/lovasz_ref.py) against fp64
autograd of the paper's Algorithm 1 written independently with torch.sort / cumsum, its known answers, the argument domains of the new
entry points and of the setter, the new bound buffers, the option's parsers, the side file, and header = _lib.py = exports.  The
kernels themselves are held by tests/test_gpu_lovasz.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lovasz_ref as LR
from drs_amd import _lib, cli, loops
from drs_amd import loops_indexed as LI
from drs_amd import patches as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the statement
def _inputs(B=3, S=13, K=6, seed=0, scale=3.0):
    rng = np.random.default_rng(seed)
    n = S * S
    lg = rng.normal(size=(B, n, K)) * scale
    y = rng.integers(0, K, size=(B, n))
    y[rng.random(size=y.shape) < 0.05] = K           # labels outside the classes
    y[0][y[0] == K - 1] = 0                           # class K - 1 absent from patch 0
    lm = (rng.random(size=y.shape) < 0.7).astype(np.uint8)       # a mask with holes
    return lg, y, lm


def _algorithm1(lg, y, K, lam, lm, inv_n):
    """Algorithm 1 of the paper with torch.sort / cumsum, classes = 'present', per patch, in fp64 with autograd"""
    lgt = torch.tensor(lg, dtype=torch.float64, requires_grad=True)
    total = torch.zeros((), dtype=torch.float64)
    for b in range(lg.shape[0]):
        keep = torch.as_tensor((y[b] < K) & (lm[b] != 0))
        if not bool(keep.any()):
            continue
        p = torch.softmax(lgt[b][keep], dim=1)
        yb = torch.as_tensor(y[b])[keep]
        losses = []
        for c in range(K):
            fg = (yb == c).to(torch.float64)
            if fg.sum() == 0:
                continue
            errs = (fg - p[:, c]).abs()
            srt, perm = torch.sort(errs, descending=True, stable=True)
            fgs = fg[perm]
            inter = fgs.sum() - fgs.cumsum(0)
            union = fgs.sum() + (1.0 - fgs).cumsum(0)
            jac = 1.0 - inter / union
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
            losses.append((srt * jac).sum())
        total = total + lam * float(keep.sum()) * torch.stack(losses).mean()
    total = total * inv_n
    total.backward()
    return float(total.detach()), lgt.grad.numpy()


def test_statement_against_autograd_of_algorithm_1():
    lg, y, lm = _inputs()
    K, lam = 6, 1.5
    r = LR.lovasz(lg, y, K, lam, loss_mask=lm)
    loss, grad = _algorithm1(lg, y, K, lam, lm, r["inv_n"])
    print("lovasz statement: loss %.3g grad %.3g" % (abs(r["loss"] - loss) / abs(loss), np.abs(r["grad"] - grad).max() / np.abs(grad).max()))
    assert abs(r["loss"] - loss) <= 1e-10 * abs(loss)
    assert np.abs(r["grad"] - grad).max() <= 1e-10 * np.abs(grad).max()
    assert not r["grad"][~r["inl"]].any()


def test_increments_are_non_negative_and_sum_to_one():
    lg, y, lm = _inputs(seed=3)
    K = 6
    r = LR.lovasz(lg, y, K, 1.0, loss_mask=lm)
    assert not r["present"][0, K - 1] and r["present"].any()
    for b in range(lg.shape[0]):
        for c in range(K):
            dj = np.abs(r["g"][b, :, c]) / max(r["factor"][b], 1e-300)
            if r["present"][b, c]:
                assert (dj >= 0).all() and abs(dj.sum() - 1.0) < 1e-12
                fg = (y[b] == c) & r["inl"][b]
                assert (r["g"][b, fg, c] < 0).all() and (r["g"][b, r["inl"][b] & ~fg, c] >= 0).all()
            else:
                assert not r["g"][b, :, c].any() and (r["rank"][b, :, c] == -1).all()
    rng = np.random.default_rng(0)
    for _ in range(50):
        fg = rng.random(rng.integers(1, 40)) < 0.4
        fg[rng.integers(0, fg.size)] = True
        dJ, F, U = LR.increments(fg)
        assert (dJ >= 0).all() and abs(dJ.sum() - 1.0) < 1e-12 and (U >= 1).all()


def test_known_answers():
    rng = np.random.default_rng(1)
    B, n, K = 2, 50, 4
    y = rng.integers(0, K, size=(B, n))
    pred = rng.integers(0, K, size=(B, n))
    # hard predictions: the loss is the mean over present classes of 1 - IoU_c
    lg = np.where(pred[..., None] == np.arange(K), 40.0, -40.0)
    r = LR.lovasz(lg, y, K, 1.0)
    for b in range(B):
        ious = []
        for c in range(K):
            if (y[b] == c).any():
                ious.append(1.0 - ((y[b] == c) & (pred[b] == c)).sum() / ((y[b] == c) | (pred[b] == c)).sum())
        assert abs(r["patch_loss"][b] / n - np.mean(ious)) < 1e-12
    # a single-class patch: the mean error
    lg = rng.normal(size=(1, n, K))
    y1 = np.full((1, n), 2)
    r = LR.lovasz(lg, y1, K, 1.0)
    assert r["C"][0] == 1 and abs(r["patch_loss"][0] / n - r["err"][0, :, 2].mean()) < 1e-12
    # one foreground pixel of class 1 among background of class 0: for class 1, the foreground pixel at position r has dJ = 1 / (1 + r),
    # a background pixel before it I / (U (U + 1)) = 1 / ((1 + r')(2 + r')), and nothing after it
    y2 = np.zeros((1, 6), dtype=np.int64)
    y2[0, 3] = 1
    err = np.zeros((1, 6, 2))
    err[0, :, 1] = [0.9, 0.1, 0.8, 0.5, 0.2, 0.3]        # order: 0, 2, 3 (foreground), 5, 4, 1
    err[0, :, 0] = 0.5
    r = LR.from_keys(err, y2, 2, 1.0)
    f = r["factor"][0]
    assert f == 6.0 / 2.0
    np.testing.assert_allclose(r["g"][0, :, 1] / f, [1.0 / 2, 0, 1.0 / 6, -1.0 / 3, 0, 0], atol=1e-15)
    assert r["rank"][0, :, 1].tolist() == [0, 5, 1, 2, 4, 3]
    assert abs(r["cls_loss"][0, 1] - (0.9 / 2 + 0.8 / 6 + 0.5 / 3)) < 1e-15


def test_absent_class_and_empty_patch_give_zeros():
    lg, y, lm = _inputs(seed=4)
    lm[2] = 0
    r = LR.lovasz(lg, y, 6, 2.0, loss_mask=lm)
    assert r["n"][2] == 0 and r["patch_loss"][2] == 0 and not r["g"][2].any() and not r["grad"][2].any() and (r["rank"][2] == -1).all()
    assert not r["g"][0, :, 5].any() and r["cls_loss"][0, 5] == 0
    r0 = LR.lovasz(lg, y, 6, 2.0, loss_mask=np.zeros_like(lm))
    assert r0["loss"] == 0 and not r0["grad"].any()


def test_shard_invariance():
    lg, y, lm = _inputs(B=4, seed=5)
    K, lam = 6, 1.5
    whole = LR.lovasz(lg, y, K, lam, loss_mask=lm)
    inv_n = whole["inv_n"]
    parts = [LR.lovasz(lg[s], y[s], K, lam, loss_mask=lm[s], inv_n=inv_n) for s in (slice(0, 2), slice(2, 4))]
    for name in ("g", "rank", "patch_loss", "grad", "cls_loss"):
        np.testing.assert_array_equal(np.concatenate([q[name] for q in parts]), whole[name])
    assert abs(parts[0]["loss"] + parts[1]["loss"] - whole["loss"]) <= 1e-15 * abs(whole["loss"])


def test_ties_resolve_to_the_lower_index():
    n, K = 12, 2
    y = np.asarray([[0, 1] * 6])
    err = np.full((1, n, K), 0.5)
    r = LR.from_keys(err, y, K, 1.0)
    assert r["rank"][0, :, 0].tolist() == list(range(n)) and r["rank"][0, :, 1].tolist() == list(range(n))
    err[0, :, 0] = [0.5, 1.0, 0.5, 1.0, 0.0, 0.0, 0.5, 1.0, 0.5, 0.0, 0.0, 2.0 ** -20]
    r = LR.from_keys(err, y, K, 1.0)
    assert r["rank"][0, :, 0].tolist() == [3, 0, 4, 1, 8, 9, 5, 2, 6, 10, 11, 7]
    lm = np.ones((1, n), dtype=np.uint8)
    lm[0, 1] = 0
    r = LR.from_keys(err, y, K, 1.0, loss_mask=lm)
    assert r["rank"][0, :, 0].tolist() == [2, -1, 3, 0, 7, 8, 4, 1, 5, 9, 10, 6]


def test_fp32_keys_follow_the_fp64_ones():
    lg, y, lm = _inputs(seed=6)
    e32 = LR.error_keys(lg.astype(np.float32), y, 6, lm, dtype=np.float32)
    e64 = LR.error_keys(lg.astype(np.float32), y, 6, lm, dtype=np.float64)
    assert e32.dtype == np.float32 and np.abs(e32 - e64).max() < 1e-6 and (e32 >= 0).all() and (e32 <= 1).all()
    assert not e32[~LR.in_loss(y, 6, lm)].any()


# ------------------------------------------------------------------------------------------------- the entry points' checks
OK, ERR_ARG, ERR_HIP = 0, 1, 2
p0, p1, p2, p3, p4, p5, p6, p7, p8 = [0x10000 + 0x1000 * i for i in range(9)]     # dummy device pointers: host code never dereferences them
NAN, INFTY = float("nan"), float("inf")
BIG = 1 << 40
CLS = [("feat", p0), ("B", 2), ("S", 16), ("P", 0), ("ld", 64), ("coff", 0), ("C", 64), ("K", 6), ("w", p1), ("bias", p2), ("labels", p3),
       ("loss_mask", None), ("acc_mask", None), ("inv_n", 1.0 / 512), ("class_weights", None), ("focal_gamma", 0.0), ("pixel_weight", None),
       ("region_grad", p4), ("logits", None), ("pred", None), ("gfeat", p5), ("ld_g", 64), ("coff_g", 0), ("dw_partial", p6), ("db_partial", p7),
       ("loss_partial", p8), ("conf", None)]
ROWS = {
    "drs_patch_lovasz_grad": (
        [("logits", p0), ("err", p1), ("labels", p2), ("loss_mask", p3), ("B", 3), ("S", 21), ("K", 6), ("lam", 1.5), ("dice_coef", p4),
         ("rank_out", p5), ("grad_out", p6), ("patch_loss_out", p7), ("scratch", p8), ("scratch_bytes", BIG)],
        [dict(err=None), dict(labels=None), dict(grad_out=None), dict(patch_loss_out=None), dict(B=0), dict(S=0), dict(B=-3), dict(S=-21),
         dict(B=1 << 12, S=64), dict(B=1, S=4096), dict(B=1 << 20, S=1 << 20), dict(K=0), dict(K=9), dict(K=-1), dict(lam=0.0), dict(lam=-1.0),
         dict(lam=64.0000001), dict(lam=NAN), dict(lam=INFTY), dict(lam=-INFTY), dict(scratch=None), dict(scratch_bytes=0),
         dict(scratch_bytes=3 * 7 * 8 - 1), dict(S=100, scratch_bytes=3 * 6 * 10000 * 16), dict(dice_coef=p4 + 4), dict(scratch=p8 + 4)],
        [dict(logits=None), dict(loss_mask=None), dict(dice_coef=None), dict(rank_out=None), dict(lam=64.0), dict(lam=1e-300), dict(K=1), dict(K=8),
         dict(B=1, S=4095), dict(B=1, S=1), dict(scratch_bytes=3 * 7 * 8 + 8), dict(S=100, scratch_bytes=3 * 6 * 10000 * 16 + 3 * 7 * 8 + 8)]),
    "drs_classifier_loss_region": (
        CLS,
        [dict(feat=None), dict(w=None), dict(bias=None), dict(K=0), dict(K=9), dict(C=32), dict(C=96), dict(B=0), dict(S=0), dict(P=-1),
         dict(inv_n=NAN), dict(inv_n=-1.0), dict(focal_gamma=NAN), dict(focal_gamma=8.5), dict(focal_gamma=-1.0), dict(B=1 << 12, S=64),
         dict(loss_partial=None), dict(dw_partial=None), dict(db_partial=None), dict(ld=62), dict(coff=2), dict(ld_g=62), dict(coff_g=4),
         dict(region_grad=p4 + 2)],
        [dict(region_grad=None), dict(labels=None, gfeat=None), dict(pixel_weight=p4), dict(focal_gamma=2.0), dict(K=2), dict(K=8), dict(gfeat=None)]),
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
    q = lambda *a: _lib.query("drs_lovasz_scratch_bytes", *a)      # noqa: E731
    assert q(3, 21, 6) == (3 * 7 * 8 + 15) // 16 * 16 and q(1, 1, 1) == 16 and q(128, 64, 6) == 128 * 7 * 8
    assert q(1, 99, 2) == 32 and q(1, 100, 2) == 32 + 2 * 10000 * 16           # the LDS form holds 9856 pixels: S <= 99
    assert q(2, 101, 8) == 2 * 9 * 8 + 2 * 8 * 10201 * 16
    for bad in ((0, 4, 2), (1, 0, 2), (1, 4, 0), (1, 4, 9), (1, 4096, 2), (-1, 4, 2)):
        assert q(*bad) == 0
    for b, s, k in ((1, 50, 2), (4, 99, 6), (4, 100, 6), (2, 300, 8)):           # monotone: a net's scratch, sized at (b_max, s_max), serves every step
        assert q(b, s, k) <= q(b + 1, s, k) and q(b, s, k) <= q(b, s + 1, k)


def test_setter_domain_getter_and_buffers():
    lib = _lib.load()
    h = C.c_void_p()
    _lib.call("drs_net_create", b"dilated_grsl", 5, 6, 0.005, 2, 17, 0, 0.5, C.byref(h))
    try:
        lam = C.c_double(-7)
        get = lambda: (lib.drs_net_get_lovasz(h, C.byref(lam)), lam.value)   # noqa: E731
        assert get() == (OK, 0.0)                                                   # never set: off
        for bad in (-0.5, -1e-300, 64.0000001, 100.0, NAN, INFTY, -INFTY):
            assert lib.drs_net_set_lovasz(h, bad) == ERR_ARG, bad
        assert get() == (OK, 0.0)                                                   # a rejected call changes nothing
        for good in (1.5, 64.0, 1e-300, 0.0, 0.25):
            assert lib.drs_net_set_lovasz(h, good) == OK
            assert get() == (OK, good)
        assert lib.drs_net_set_lovasz(h, NAN) == ERR_ARG and get() == (OK, 0.25)    # ... nor when a value is in use
        assert lib.drs_net_get_lovasz(h, None) == OK
        assert lib.drs_net_set_lovasz(None, 1.0) == ERR_ARG and lib.drs_net_get_lovasz(None, None) == ERR_ARG
        name, nb, dt = C.create_string_buffer(64), C.c_size_t(), C.c_int()
        info, names = {}, []
        for i in range(_lib.query("drs_net_num_buffers", h)):
            _lib.call("drs_net_buffer_info", h, i, name, 64, C.byref(nb), C.byref(dt))
            info[name.value.decode()] = (nb.value, dt.value)
            names.append(name.value.decode())
        M, K, B = 2 * 17 * 17, 6, 2
        f32, f64 = info["pixel_weight"][1], info["dice_loss"][1]
        assert info["lovasz_err"] == (4 * M * K, f32) and info["region_grad"] == (4 * M * K, f32) and info["lovasz_loss"] == (8 * B, f64)
        assert info["lovasz_scratch"] == (_lib.query("drs_lovasz_scratch_bytes", B, 17, K), f64)
        i = names.index("hard_ce")
        assert names[i + 1:i + 6] == ["lovasz_err", "region_grad", "lovasz_loss", "lovasz_scratch", "logits"]      # directly after hard_ce
        assert names[-1] == "pixel_weight" and names[-2] == "loss_mask"
    finally:
        lib.drs_net_destroy(h)
    assert _lib.query("drs_net_num_timing_kinds") == 15


# ------------------------------------------------------------------------------------------------- the option
def test_check_lovasz():
    assert P.check_lovasz(1.5) == 1.5 and P.check_lovasz((2,)) == 2.0 and P.check_lovasz(0) == 0.0 and P.check_lovasz([64]) == 64.0
    assert P.check_lovasz(np.float32(0.5)) == 0.5 and type(P.check_lovasz(np.int64(3))) is float
    for bad in (-0.1, 64.5, NAN, INFTY, "1", None, True, (1, 2), (), [np.bool_(1)], 1 + 2j):
        with pytest.raises(ValueError):
            P.check_lovasz(bad)


def test_parse_lovasz():
    assert P.parse_lovasz("1.5") == 1.5 and P.parse_lovasz("0") == 0.0 and P.parse_lovasz("2.5e-1") == 0.25 and P.parse_lovasz("64") == 64.0
    for bad in ("", " 1", "1 ", "1,2", "x", "65", "-1", "nan", "inf", "1,"):
        with pytest.raises(ValueError):
            P.parse_lovasz(bad)


def test_cli_flag():
    base = ["prog", "a", "b"]
    assert cli.parse_lovasz(base) == (base, None)
    assert cli.parse_lovasz(base + ["--lovasz-weight=1.5"]) == (base, 1.5)
    assert cli.parse_lovasz(["prog", "--lovasz-weight=0", "a", "b"]) == (base, 0.0)
    for arg in ("--lovasz-weight", "--lovasz-weight=", "--lovasz-weight=65", "--lovasz-weight=1,2", "--lovasz-weight=x"):
        with pytest.raises(ValueError, match="expected --lovasz-weight=lam"):
            cli.parse_lovasz(["prog", "a", arg])
    with pytest.raises(ValueError, match="more than once"):
        cli.parse_lovasz(["prog", "--lovasz-weight=0.5", "x", "--lovasz-weight=0.5"])
    for fn in (loops.train, LI.train):
        assert inspect.signature(fn).parameters["lovasz"].default is None
        assert "setup_lovasz(net, lovasz, comm, say)" in inspect.getsource(fn) and "Lovasz" in fn.__doc__
    assert inspect.getsource(cli).count("lovasz=lovasz") == 3
    assert inspect.getsource(cli).count("argv, lovasz = parse_lovasz(argv)") == 3
    assert "save_lovasz(net, output_path, step)" in inspect.getsource(LI.train)
    assert "--lovasz-weight=lam" in cli.__doc__


class _Net(object):
    """what save_checkpoint / load_checkpoint / setup_lovasz touch of a net"""

    def __init__(self):
        self._l = None

    def state_dict(self):
        return {"w": np.zeros(2, dtype=np.float32)}

    def load_state_dict(self, d):
        pass

    def set_lovasz(self, v):
        self._l = None if v is None else P.check_lovasz(v)

    @property
    def lovasz(self):
        return None if self._l is None or self._l == 0.0 else self._l


def test_side_file_round_trip(tmp_path, capsys):
    out = str(tmp_path) + os.sep
    a = _Net()
    a.set_lovasz(0.1)
    loops.save_checkpoint(a, out, 1000)
    assert os.path.isfile(out + "lovasz_step_1000.npy")
    side = np.load(out + "lovasz_step_1000.npy")
    assert side.dtype == np.float64 and side.tolist() == [0.1]
    b = _Net()
    loops.load_checkpoint(b, out + "model-1000")
    assert "Lovasz term (restored from " + out + "lovasz_step_1000.npy): lambda 0.1" in capsys.readouterr().out
    assert b.lovasz == a.lovasz == 0.1
    a.set_lovasz(0)
    loops.save_checkpoint(a, out, 7)
    assert not os.path.exists(out + "lovasz_step_7.npy")             # lam = 0 is unset
    b = _Net()
    loops.load_checkpoint(b, out + "model-7")
    assert b.lovasz is None and "Lovasz" not in capsys.readouterr().out


def test_setup_lovasz_overrides_and_says_so():
    from drs_amd.net import NoComm
    net, lines = _Net(), []
    assert loops.setup_lovasz(net, 0, NoComm(), lines.append) == 0.0 and lines == [] and net.lovasz is None
    assert loops.setup_lovasz(net, 1.5, NoComm(), lines.append) == 1.5 and net.lovasz == 1.5
    assert len(lines) == 1 and lines[0].startswith("Lovasz term: lambda 1.5") and "replacing" not in lines[0]
    loops.setup_lovasz(net, 0.5, NoComm(), lines.append)
    assert net.lovasz == 0.5 and "replacing the value restored from the checkpoint, lambda 1.5" in lines[1]
    loops.setup_lovasz(net, 0, NoComm(), lines.append)
    assert net.lovasz is None and len(lines) == 3 and "lambda 0 (off" in lines[2] and "replacing" in lines[2]
    with pytest.raises(ValueError):
        loops.setup_lovasz(net, 65, NoComm(), lines.append)

    class TwoRanks(NoComm):
        def agree(self, values, what):
            self.seen = (list(values), what)
    comm = TwoRanks()
    loops.setup_lovasz(net, 0.3, comm, lines.append)
    assert comm.seen == (np.asarray([0.3], dtype=np.float64).view(np.uint32).tolist(), "lovasz term")


def test_both_nets_carry_the_option():
    from drs_amd import engine, net, oplevel
    for cls in (engine.EngineNet, oplevel.OpLevelNet):
        assert isinstance(inspect.getattr_static(cls, "lovasz"), property) and hasattr(cls, "set_lovasz")
    assert "not mined" in net.DilatedNet.set_lovasz.__doc__ and "inspection" in loops.lovasz_grad.__doc__


# ------------------------------------------------------------------------------------------------- header, signatures, exports
def test_header_lib_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    new = ("drs_lovasz_scratch_bytes", "drs_patch_lovasz_grad", "drs_classifier_loss_region", "drs_net_set_lovasz", "drs_net_get_lovasz")
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
    assert hdr.index("int drs_patch_lovasz_grad(") > hdr.index(" * Training level: Lovasz-softmax term (opt-in") > hdr.index("int drs_patch_hard_weight(") > step
    assert step < hdr.index("int drs_net_get_hard_mining(") < hdr.index("int drs_net_set_lovasz(") < hdr.index("int drs_net_get_lovasz(") < hdr.index("Whole-map level")
    sig = _lib.SIGNATURES["drs_patch_lovasz_grad"][1]
    assert sig[7] is C.c_double and sig[13] is C.c_size_t and _lib.SIGNATURES["drs_net_set_lovasz"][1][1:] == [C.c_double]
    assert _lib.SIGNATURES["drs_classifier_loss_region"][1] == _lib.SIGNATURES["drs_classifier_loss_dice"][1]
    assert _lib.SIGNATURES["drs_lovasz_scratch_bytes"][0] is C.c_size_t
