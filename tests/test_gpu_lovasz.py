"""-m gpu: the Lovasz-softmax term of the training loss from the kernels up: the keys of drs_patch_lovasz_grad against
the fp32 formula, its order bit for bit against the numpy statement (tests/lovasz_ref.py, itself held by tests/test_lovasz_plan.py) on
the device's own keys, the map and the patches' terms against fp64 at those ranks, the three forms of the fused classifier with a map
against the fp64 closed form and, with the Dice coefficients expanded, bit for bit against drs_classifier_loss_dice, the bitwise no-ops,
a whole training step against fp64 autograd, engine = op level, lam = 0, two ranks, the training loop and the three command lines.

Tolerances are the project's existing ones: single ops 1e-5 relative to the tensor's maximum and 1e-6 for a loss, whole nets 1e-4
(logits 1e-3), two ranks as tests/test_gpu_dp.py.  A patch's term (lam n_b / C_b) sum_c Loss_bc has the scale lam n_b (every Loss_bc
lies in [0, 1]), so its 1e-12 and 1e-6 are relative to the reference value: two fp64 sums of at most 10^4 terms in different fixed
orders differ by at most 10^4 2^-53 = 1.1e-12 of it."""
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import boundary_weight_ref as BR   # noqa: E402
import lovasz_ref as LR   # noqa: E402
from gpu_util import DEV, dev, rel_err, stream   # noqa: E402
from test_gpu_class_weights import WEIGHTS, _feed_step, _ForcedTorchNet   # noqa: E402  (helpers only)
from test_gpu_focal_loss import FORMS, _check_form, _moderate   # noqa: E402  (helpers only: the form table, its shared inputs)
from test_gpu_dice_loss import _Dc, _coefficients_of, _mode, _step_inputs, _torch_dice, MODES, STEP_CASES, DICE, BW   # noqa: E402  (helpers only)

HM = (0.25, 16)
MARK = -7.0


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# ------------------------------------------------------------------------------------------------- the pre-pass kernel
# (1, 99, 2) and (1, 100, 2): the largest side whose patch stays in LDS (9801 <= 9856 pixels) and the smallest that goes through scratch
SHAPES = [(1, 1, 2), (2, 13, 3), (3, 16, 6), (2, 37, 8), (1, 70, 6), (1, 99, 2), (1, 100, 2)]
LAMS = {1: 1.0, 13: 2.5, 16: 1.5, 37: 64.0, 70: 0.75, 99: 1.5, 100: 1.5}
G = 64          # guard words around every output


def _inputs(B, S, K, seed):
    """name -> (logits float32 [B, S S, K] or None, err float32 [B, S S, K] or None, labels uint8 [B, S S], loss mask uint8 or None).
    "mixed": a loss mask with holes, labels >= K, class K - 1 absent from patch 0, and (B > 1) a last patch with no pixel in the loss;
    "no-mask"; "nothing-in-the-loss"; "ties": logits NULL, err drawn from {+0, 2^-20, 0.5, 1.0}; "all-equal": every key 0.5"""
    rng = np.random.default_rng(seed)
    n = S * S
    lg = (rng.normal(size=(B, n, K)) * 3.0).astype(np.float32)
    y = rng.integers(0, K, size=(B, n)).astype(np.uint8)
    out = rng.random(size=y.shape) < 0.05
    y[out] = rng.choice([K, 255], size=int(out.sum())).astype(np.uint8)
    y[0][y[0] == K - 1] = 0
    lm = (rng.random(size=y.shape) < 0.7).astype(np.uint8)
    if n > 1:
        lm[0, 0], y[0, 0] = 1, 0                       # (patch 0 keeps a pixel in the loss)
    if B > 1:
        lm[B - 1] = 0
    ties = rng.choice(np.asarray([0.0, 2.0 ** -20, 0.5, 1.0], dtype=np.float32), size=(B, n, K))
    return {"mixed": (lg, None, y, lm), "no-mask": (lg, None, y, None), "nothing-in-the-loss": (lg, None, y, np.zeros_like(lm)),
            "ties": (None, ties, y, lm), "all-equal": (None, np.full((B, n, K), 0.5, dtype=np.float32), y, None)}


class _Pre(object):
    """one call of drs_patch_lovasz_grad with guard words around every output"""

    def __init__(self, lib, lg, err, y, lm, B, S, K, lam, dice=None, want_rank=True, scratch_fill=0):
        M = B * S * S
        self.lgd = None if lg is None else dev(lg.reshape(-1))
        self.err = torch.full((M * K + 2 * G,), MARK, dtype=torch.float32, device=DEV)
        if err is not None:
            self.err[G:G + M * K] = dev(err.reshape(-1))
        self.yd, self.lmd = dev(y.reshape(-1)), None if lm is None else dev(lm.reshape(-1))
        self.rank = torch.full((M * K + 2 * G,), 12345, dtype=torch.int32, device=DEV) if want_rank else None
        self.grad = torch.full((M * K + 2 * G,), MARK, dtype=torch.float32, device=DEV)
        self.pl = torch.full((B + 2 * G,), MARK, dtype=torch.float64, device=DEV)
        nbytes = lib.query("drs_lovasz_scratch_bytes", B, S, K)
        assert nbytes > 0 and nbytes % 16 == 0
        self.scratch = torch.full((nbytes + 2 * G,), scratch_fill, dtype=torch.uint8, device=DEV)
        self.dice = None if dice is None else dev(dice.reshape(-1).astype(np.float32))
        lib.call("drs_patch_lovasz_grad", None if self.lgd is None else self.lgd.data_ptr(), self.err[G:].data_ptr(), self.yd.data_ptr(),
                 None if self.lmd is None else self.lmd.data_ptr(), B, S, K, lam, None if self.dice is None else self.dice.data_ptr(),
                 None if self.rank is None else self.rank[G:].data_ptr(), self.grad[G:].data_ptr(), self.pl[G:].data_ptr(),
                 self.scratch[G:].data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        self.shape, self.nbytes = (B, S * S, K), nbytes

    def host(self):
        B, n, K = self.shape
        M = B * n
        rk = None if self.rank is None else self.rank[G:G + M * K].cpu().numpy().view(np.uint32).astype(np.int64).reshape(B, n, K)
        if rk is not None:
            rk[rk == 0xFFFFFFFF] = -1
        return (self.err[G:G + M * K].cpu().numpy().reshape(B, n, K), rk, self.grad[G:G + M * K].cpu().numpy().reshape(B, n, K),
                self.pl[G:G + B].cpu().numpy())

    def guards_ok(self):
        B, n, K = self.shape
        M = B * n
        ok = bool((self.err[:G] == MARK).all() and (self.err[G + M * K:] == MARK).all() and (self.grad[:G] == MARK).all() and
                  (self.grad[G + M * K:] == MARK).all() and (self.pl[:G] == MARK).all() and (self.pl[G + B:] == MARK).all())
        if self.rank is not None:
            ok = ok and bool((self.rank[:G] == 12345).all() and (self.rank[G + M * K:] == 12345).all())
        return ok


@pytest.mark.parametrize("B,S,K", SHAPES, ids=["%dx%dx%d-K%d" % (b, s, s, k) for b, s, k in SHAPES])
def test_prepass_against_the_statement(lib, B, S, K):
    lam = LAMS[S]
    n = S * S
    assert (lib.query("drs_lovasz_scratch_bytes", B, S, K) > 16 * B * K * n) == (S >= 100)          # which storage form this shape takes
    for name, (lg, err_in, y, lm) in _inputs(B, S, K, seed=100 * S + K).items():
        r = _Pre(lib, lg, err_in, y, lm, B, S, K, lam)
        err, rank, grad, pl = r.host()
        inl = LR.in_loss(y, K, lm)
        assert r.guards_ok(), name
        if lg is not None:
            # the keys against the fp32 formula (numpy's exp is not the device's expf: 1e-6 absolute), +0 outside the loss
            want = LR.error_keys(lg, y, K, lm, dtype=np.float32)
            e_key = float(np.abs(err.astype(np.float64) - want).max())
            assert e_key < 1e-6 and not err[~inl].any() and (err >= 0).all() and (err <= 1).all(), (name, e_key)
        else:
            np.testing.assert_array_equal(err, err_in)                                  # the input is left as it came
        # the order: exactly the statement's on the device's own keys
        ref = LR.from_keys(err, y, K, lam, lm)
        if name == "mixed" and S > 1:
            assert (y >= K).any() and not ref["present"][0, K - 1] and ref["n"][0] > 0 and (B == 1 or ref["n"][B - 1] == 0)
        if name == "nothing-in-the-loss":
            assert not ref["n"].any()
        np.testing.assert_array_equal(rank, ref["rank"], err_msg=name)
        # the map: within one fp32 rounding of the fp64 value at those ranks, right signs, exact zeros outside the loss and at absent classes
        g = ref["g"]
        assert (np.abs(grad.astype(np.float64) - g) <= 2.0 ** -23 * np.abs(g)).all(), name
        fg = (y[..., None] == np.arange(K)) & inl[..., None]
        assert (grad[fg & ref["present"][:, None, :]] < 0).all() and (grad[~fg] >= 0).all() and not grad[~inl].any()
        assert not np.signbit(grad[~inl]).any() and not grad[np.broadcast_to(~ref["present"][:, None, :], grad.shape)].any()
        # the patches' terms: 1e-12 on the device's own keys; 1e-6 of the fp64 statement on the logits path
        e_pl = np.abs(pl - ref["patch_loss"])
        assert (e_pl <= 1e-12 * np.abs(ref["patch_loss"])).all(), (name, e_pl)
        if lg is not None:
            full = LR.lovasz(lg.astype(np.float64), y, K, lam, loss_mask=lm, order_keys=err)
            assert (np.abs(pl - full["patch_loss"]) <= 1e-6 * np.abs(full["patch_loss"])).all(), name
        empty = ref["n"] == 0
        assert not grad[empty].any() and not pl[empty].any() and (rank[empty] == -1).all()
        print("lovasz pre-pass %dx%dx%d K%d %s: patch_loss %.3g" % (B, S, S, K, name, float((e_pl / np.maximum(np.abs(ref["patch_loss"]), 1e-300)).max())))
        # rank_out = NULL gives the same outputs, a second run the same bits, and scratch full of 0xFF bytes the same bits as zeroed scratch
        r2 = _Pre(lib, lg, err_in, y, lm, B, S, K, lam, want_rank=False)
        r3 = _Pre(lib, lg, err_in, y, lm, B, S, K, lam, scratch_fill=0xFF)
        for other in (r2, r3):
            assert torch.equal(other.grad, r.grad) and torch.equal(other.pl, r.pl) and torch.equal(other.err, r.err) and other.guards_ok()
            assert (other.scratch[:G] == other.scratch[0]).all() and (other.scratch[G + other.nbytes:] == other.scratch[0]).all()
        assert torch.equal(r3.rank, r.rank)


def test_prepass_folds_the_dice_coefficients_in_with_one_add(lib):
    B, S, K = 3, 16, 6
    lg, _, y, lm = _inputs(B, S, K, seed=9)["mixed"]
    rng = np.random.default_rng(9)
    coef = np.stack([-rng.random((B, K)), rng.random((B, K))], axis=2).astype(np.float32)
    a, b = _Pre(lib, lg, None, y, lm, B, S, K, 1.5), _Pre(lib, lg, None, y, lm, B, S, K, 1.5, dice=coef)
    _, rank_a, ga, pla = a.host()
    _, rank_b, gb, plb = b.host()
    inl = LR.in_loss(y, K, lm)
    onehot = y[..., None] == np.arange(K)
    want = ga + np.where(onehot, coef[:, None, :, 0], coef[:, None, :, 1])
    want[~inl] = 0
    np.testing.assert_array_equal(gb, want)
    np.testing.assert_array_equal(rank_a, rank_b)
    np.testing.assert_array_equal(pla, plb)
    assert gb[0, inl[0], K - 1].any() and (rank_b[0, :, K - 1] == -1).all()          # an absent class still carries its Dice part


def test_loops_lovasz_grad_returns_the_map_and_the_ranks(lib):
    from drs_amd import loops
    B, S, K = 2, 13, 3
    lg, _, y, lm = _inputs(B, S, K, seed=4)["mixed"]
    grad, rank, err, pl = loops.lovasz_grad(lg.reshape(B, S, S, K), y.reshape(B, S, S), 2.5, loss_mask=lm.reshape(B, S, S))
    r = _Pre(lib, lg, None, y, lm, B, S, K, 2.5)
    e2, rk2, g2, pl2 = r.host()
    np.testing.assert_array_equal(grad.cpu().numpy().reshape(B, -1, K), g2)
    np.testing.assert_array_equal(rank.cpu().numpy().reshape(B, -1, K), rk2)
    np.testing.assert_array_equal(err.cpu().numpy().reshape(B, -1, K), e2)
    np.testing.assert_array_equal(pl.cpu().numpy(), pl2)


# ------------------------------------------------------------------------------------------------- the classifier with a map
LAM = 1.5
LMODES = {"alone": MODES["dice-alone"], "on-weights-focal-map": MODES["on-weights-focal-map"]}


class _Rg(_Dc):
    """one launch of drs_classifier_loss_region and its slab reductions: test_gpu_dice_loss._Dc with the map in the coefficients' place"""

    def __init__(self, lib, d, form, wc, gamma, pw, region, labels=True):
        real = lib.call

        def call(entry, *args):
            real("drs_classifier_loss_region" if entry == "drs_classifier_loss_dice" else entry, *args)
        shim = type("Shim", (), {"call": staticmethod(call), "query": staticmethod(lib.query)})
        _Dc.__init__(self, shim, d, form, wc, gamma, pw, region, labels=labels)


def _region_of(lib, d, form, dice=None):
    """the step's pre-pass on the form's inputs: the map from the logits of the plain launch (+ the Dice coefficients when given)"""
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    err = torch.zeros(M * K, dtype=torch.float32, device=DEV)
    grad = torch.zeros(M * K, dtype=torch.float32, device=DEV)
    pl = torch.zeros(B, dtype=torch.float64, device=DEV)
    nbytes = lib.query("drs_lovasz_scratch_bytes", B, S, K)
    scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
    lib.call("drs_patch_lovasz_grad", d["plain"].logits.data_ptr(), err.data_ptr(), d["yd"].data_ptr(), d["lmd"].data_ptr(), B, S, K, LAM,
             None if dice is None else dice.data_ptr(), None, grad.data_ptr(), pl.data_ptr(), scratch.data_ptr(), nbytes, stream())
    torch.cuda.synchronize()
    return grad, pl, err


LCASES = [(f, m) for f in FORMS for m in LMODES]


@pytest.mark.parametrize("form,mode", LCASES, ids=["%s-%s" % c for c in LCASES])
def test_region_classifier_against_fp64_numpy(lib, form, mode):
    """the structure and tolerances of tests/test_gpu_dice_loss.py::test_dice_classifier_against_fp64_numpy; the order of every
    (patch, class) is the device's (its fp32 keys through the statement): the surrogate is piecewise linear"""
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    d = _moderate(form)
    wc, gamma, pw = _mode(form, "dice-alone" if mode == "alone" else mode)
    yy, inl = d["yy"], d["inl"]
    wc64 = np.ones(K) if wc is None else wc.astype(np.float64)
    pw64 = np.ones(M) if pw is None else pw.astype(np.float64)
    ce = BR.pixel_weighted_closed_form(d["lg_ref"], np.minimum(yy, K - 1), wc64, gamma, pw64)
    ce_loss = float((ce["term"] * inl).sum() / d["n"])
    gl_ce = ce["grad"] * (inl / d["n"])[:, None]
    lm = d["lmd"].cpu().numpy().reshape(B, S * S)
    region, pl, err = _region_of(lib, d, form)
    lv = LR.lovasz(d["lg_ref"].reshape(B, S * S, K), yy.reshape(B, S * S), K, LAM, loss_mask=lm, inv_n=1.0 / d["n"],
                   order_keys=err.cpu().numpy().reshape(B, S * S, K))
    np.testing.assert_array_equal(lv["inl"].reshape(-1), inl)
    gl = gl_ce + lv["grad"].reshape(M, K)
    w64, f64 = d["w64"], d["f64"]
    gf_ce, gf = gl_ce @ w64.T, gl @ w64.T
    share = float(np.linalg.norm(gf - gf_ce) / np.linalg.norm(gf_ce))
    assert share > 1e-2, share                          # the term changes gfeat by more than 1 % in norm
    r = _Rg(lib, d, form, wc, gamma, None if pw is None else dev(pw), region)
    plain = d["plain"]
    assert torch.equal(r.logits, plain.logits) and torch.equal(r.pred, plain.pred) and torch.equal(r.conf, plain.conf)
    figures = dict(ce_loss=abs(r.ls.item() / d["n"] - ce_loss) / abs(ce_loss),
                   loss=abs((r.ls.item() + pl.sum().item()) / d["n"] - (ce_loss + lv["loss"])) / abs(ce_loss + lv["loss"]),
                   lovasz_loss=abs(pl.sum().item() / d["n"] - lv["loss"]) / abs(lv["loss"]),
                   gfeat=rel_err(r.gfeat.cpu().numpy().reshape(M, C), gf), dw=rel_err(r.dw.cpu().numpy().reshape(C, K), f64.T @ gl),
                   db=rel_err(r.db.cpu().numpy(), gl.sum(axis=0)), share=share)
    print("region classifier %s %s: %s" % (form, mode, figures))
    assert not r.gfeat.view(M, C)[torch.from_numpy(~inl).to(DEV)].any()          # not in the loss: exact zeros
    assert np.isfinite(r.gfeat.cpu().numpy()).all()
    assert figures["ce_loss"] < 1e-6 and figures["loss"] < 1e-6 and figures["lovasz_loss"] < 1e-6
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5


@pytest.mark.parametrize("form", list(FORMS))
def test_no_map_and_no_labels_are_bitwise_the_pixel_call_and_expanded_dice_is_bitwise_the_dice_call(lib, form):
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    d = _moderate(form)
    region, _, _ = _region_of(lib, d, form)
    coef, _ = _coefficients_of(lib, d, form, 0.3, 0.7)
    onehot = (d["yd"].view(M, 1).to(torch.int64) == torch.arange(K, device=DEV).view(1, K))
    cf = coef.view(B, 1, K, 2).expand(B, S * S, K, 2).reshape(M, K, 2)
    expanded = torch.where(onehot, cf[..., 0], cf[..., 1]).contiguous().view(-1)          # g[p][c] = y == c ? G_in : G_out
    for mode in MODES:
        wc, gamma, pw = _mode(form, mode)
        pwd = None if pw is None else dev(pw)
        base = _Dc(lib, d, form, wc, gamma, pwd, None, entry="drs_classifier_loss_pixel")
        assert float(base.gfeat.abs().max()) > 0 and float(base.ls.item()) > 0
        r = _Rg(lib, d, form, wc, gamma, pwd, None)
        for name in _Dc.RAW + ("dw", "db", "ls"):
            assert torch.equal(getattr(r, name), getattr(base, name)), (name, mode)
        # a map changes the gradients; the cross-entropy sum, the logits, the arg-max and the confusion matrix keep their bits
        r = _Rg(lib, d, form, wc, gamma, pwd, region)
        assert not torch.equal(r.gfeat, base.gfeat) and not torch.equal(r.dw, base.dw)
        for name in ("logits", "pred", "conf", "lp", "ls"):
            assert torch.equal(getattr(r, name), getattr(base, name)), (name, mode)
        # labels == NULL is an inference launch: the map is not read
        a = _Rg(lib, d, form, wc, gamma, pwd, region, labels=False)
        b = _Dc(lib, d, form, wc, gamma, pwd, None, entry="drs_classifier_loss_pixel", labels=False)
        assert torch.equal(a.logits, b.logits) and torch.equal(a.pred, b.pred) and torch.equal(a.logits, d["plain"].logits)
        # the Dice coefficients expanded per pixel: bit for bit drs_classifier_loss_dice with those coefficients
        want = _Dc(lib, d, form, wc, gamma, pwd, coef)
        got = _Rg(lib, d, form, wc, gamma, pwd, expanded)
        for name in _Dc.RAW + ("dw", "db", "ls"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (name, mode)


# ------------------------------------------------------------------------------------------------- the step
LOV = 1.5


def _torch_lovasz(logits, y, K, lam, n_glob, rank, mask=None):
    """L_lov written with torch ops, patch by patch and class by class: the errors |[y = c] - p_c| gathered in the given order (rank
    [B, n, K], -1 = not in the loss / absent), times the Jaccard increments of that order as constants"""
    B = logits.shape[0]
    total = 0.0
    for b in range(B):
        p = torch.softmax(logits[b].reshape(-1, K), dim=1)
        yb = y[b].reshape(-1)
        inl = np.ones(yb.shape, dtype=bool) if mask is None else mask[b].reshape(-1) != 0
        present = [c for c in range(K) if ((yb == c) & inl).any()]
        per_class = 0.0
        for c in present:
            rk = rank[b, :, c]
            o = np.argsort(np.where(rk < 0, 1 << 40, rk), kind="stable")[:int(inl.sum())]
            assert (rk[o] == np.arange(o.size)).all()
            fg = yb[o] == c
            dJ, _, _ = LR.increments(fg)
            e = (torch.as_tensor(fg.astype(np.float64)) - p[torch.as_tensor(o), c]).abs()
            per_class = per_class + (e * torch.as_tensor(dJ)).sum()
        if present:
            total = total + lam * float(inl.sum()) / len(present) * per_class
    return total / n_glob


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES, ids=["Dilated6Pooling", "DenseDilated6"])
def test_lovasz_step_against_fp64_autograd(net, ch, K, B, S):
    """on top of class weights, the focal factor, the boundary weight, the Dice term and hard mining.  Decision-aligned as the
    project's step tests are: ReLU signs, pool winners and the mined weight map from the device, and the order of every (patch,
    class) from the device's fp32 logits through the numpy statement"""
    from drs_amd import loops
    from drs_amd.net import DilatedNet
    WD, GAMMA = 0.005, 2.0
    M = B * S * S
    d = DilatedNet(net, ch, K, WD, b_max=B, s_max=S, device=DEV, seed=11)
    x, y, valid = _step_inputs(ch, K, B, S, 11)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32) + 0.25
    d.set_class_weights(wc)
    d.set_focal_gamma(GAMMA)
    d.set_boundary_weight(BW)
    d.set_dice(DICE)
    d.set_hard_mining(HM)
    d.set_lovasz(LOV)
    assert d.lovasz == LOV and d.dice == DICE and d.hard_mining == HM
    params = {n: d.get_variable(n).astype(np.float64) for n in d.variable_names()}
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S, acc_mask=valid.reshape(B, -1))
    out = d.train_step(B, S, 0.01, apply_update=False, want_logits=True)
    torch.cuda.synchronize()
    # the map the step left = a direct call on the step's logits with the step's Dice coefficients
    g2, rank, err2, pl2 = loops.lovasz_grad(d.logits[:M * K].view(B, S, S, K), d.labels[:M].view(B, S, S), LOV, dice_coef=d.dice_coef[:B * K * 2].view(B, K, 2))
    assert torch.equal(g2.reshape(-1), d.region_grad[:M * K]) and torch.equal(err2.reshape(-1), d.lovasz_err[:M * K])
    assert torch.equal(pl2, d.lovasz_loss[:B])
    rank = rank.cpu().numpy().reshape(B, S * S, K)
    np.testing.assert_array_equal(rank, LR.from_keys(err2.cpu().numpy().reshape(B, S * S, K), y.reshape(B, -1), K, LOV)["rank"])
    w_step = d.pixel_weight[:M].cpu().numpy().astype(np.float64)
    dec = []
    for i, L in enumerate(d.plan.layers):
        z = d.z[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        mr = d.mean_rstd[i].cpu().numpy().reshape(L.cout, 2)
        dcs = {"pos": (z - mr[:, 0]) * mr[:, 1] > 0}
        if d._is_max(i):
            dcs["idx"] = d.idx[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        dec.append(dcs)

    def total(tn):
        for q in tn.params_list():
            q.grad = None
        logits = tn.forward(x.astype(np.float64), True)
        yy = torch.as_tensor(y.reshape(-1), dtype=torch.long)
        logp = torch.log_softmax(logits.reshape(-1, K), dim=1).gather(1, yy[:, None])[:, 0]
        l2 = sum(0.5 * (w_ ** 2).sum() for w_ in list(tn.w.values()) + list(tn.fcw.values()))
        term = torch.as_tensor(wc, dtype=torch.float64)[yy] * (1.0 - torch.exp(logp)) ** GAMMA * (-logp)
        ce = (torch.as_tensor(w_step) * term).sum() / M
        lg_nhwc = logits if logits.shape[-1] == K else logits.permute(0, 2, 3, 1)
        lov = _torch_lovasz(lg_nhwc, y, K, LOV, M, rank)
        loss = ce + _torch_dice(lg_nhwc, y, K, DICE, M) + lov + WD * l2
        loss.backward()
        return float(loss.detach()), logits.detach().numpy(), float(lov.detach())
    forced = _ForcedTorchNet(net, ch, K, params=params, dtype=torch.float64)
    forced.dec = dec
    loss_ref, logits_ref, lov_part = total(forced)
    got_loss = d.loss_value(out["loss_parts"])
    print("lovasz step %s: loss %.9g forced %.9g (the Lovasz term %.9g)" % (net, got_loss, loss_ref, lov_part))
    assert lov_part > 1e-2 * (loss_ref - lov_part)
    assert abs(got_loss - loss_ref) < 1e-4 * abs(loss_ref)
    lg = d.logits[:M * K].cpu().numpy().reshape(B, S, S, K)
    assert rel_err(lg, logits_ref) < 1e-3
    conv_names = {L.name for L in d.plan.layers}
    for name in d.plan.offsets:
        scope, kind = name.rsplit("/", 1)
        got = d.get_gradient(name).astype(np.float64)
        if kind == "weights":
            got = got + WD * d.get_variable(name)           # the decay term is applied inside the update kernel
            want = np.transpose(forced.w[scope].grad.numpy(), (2, 3, 1, 0)).reshape(got.shape)
        else:
            want = forced.b[scope].grad.numpy()
        if kind == "biases" and scope in conv_names:
            assert np.abs(want).max() < 1e-9 and np.all(got == 0)
            continue
        e = rel_err(got, want)
        print("  %s %.3g" % (name, e))
        assert e < 1e-4, name
    cm = np.zeros((K, K), dtype=np.int64)
    ok = valid.reshape(-1) != 0
    np.add.at(cm, (y.reshape(-1)[ok], out["pred"].cpu().numpy().reshape(-1)[ok]), 1)
    np.testing.assert_array_equal(out["conf"].cpu().numpy().reshape(K, K), cm)
    # an eval forward ignores the option
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S)
    _, l1 = d.forward(B, S)
    l1 = l1.clone()
    d.set_lovasz(None)
    _, l0 = d.forward(B, S)
    assert torch.equal(l0, l1)


def test_lovasz_step_with_a_loss_mask_counts_patches_by_their_valid_pixels():
    """contest's void mask: the step's term against the numpy statement on the step's own logits, global_pixels = the unmasked count"""
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    d = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=5)
    x, y, _ = _step_inputs(ch, K, B, S, 5)
    rng = np.random.default_rng(5)
    mask = (rng.random((B, S * S)) < 0.6).astype(np.uint8)
    mask[1] = 0                                       # a patch that is all void
    n = int(mask.sum())
    losses = {}
    for lam in (None, LOV):
        d.set_lovasz(lam)
        d.feed(x.reshape(B, -1), y.reshape(B, -1), S, mask=mask)
        out = d.train_step(B, S, 0.01, use_loss_mask=True, global_pixels=n, apply_update=False, want_logits=True)
        torch.cuda.synchronize()
        losses[lam] = float(out["loss_parts"][0].item())
    lg = d.logits[:B * S * S * K].cpu().numpy().astype(np.float64).reshape(B, S * S, K)
    ref = LR.lovasz(lg, y.reshape(B, -1), K, LOV, loss_mask=mask, inv_n=1.0 / n,
                    order_keys=d.lovasz_err[:B * S * S * K].cpu().numpy().reshape(B, S * S, K))
    assert ref["n"][1] == 0 and ref["patch_loss"][1] == 0 and ref["loss"] > 1e-2 * losses[None]
    print("lovasz step with a loss mask: %.9g = %.9g + %.9g" % (losses[LOV], losses[None], ref["loss"]))
    assert abs(losses[LOV] - losses[None] - ref["loss"]) < 1e-6 * losses[LOV]
    assert not d.region_grad[:B * S * S * K].view(B, S * S, K)[1].any() and d.lovasz_loss[1].item() == 0


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES)
def test_step_engine_equals_op_level_and_repeats_bitwise(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    from drs_amd.engine import EngineNet
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    nets = [mk(), mk(engine=False), mk(), mk(), mk(engine=False)]
    assert isinstance(nets[0], EngineNet) and not isinstance(nets[1], EngineNet)
    for d in nets[:3]:                       # on top of class weights, the focal term, the boundary weight, the Dice term and mining ...
        d.set_class_weights(WEIGHTS[K])
        d.set_focal_gamma(2.0)
        d.set_boundary_weight(BW)
        d.set_dice(DICE)
        d.set_hard_mining(HM)
    for d in nets:                           # ... and alone
        d.set_lovasz(LOV)
        assert d.lovasz == LOV
    off = mk()
    n = B * S * S * K
    for step in range(2):
        x, y, valid = _step_inputs(ch, K, B, S, 20 + step)
        feed = lambda d, **kw: (d.feed(x.reshape(B, -1), y.reshape(B, -1), S, acc_mask=valid.reshape(B, -1)), d.train_step(B, S, 0.01, **kw))[1]   # noqa: E731
        outs = [feed(d, want_logits=True) for d in nets]
        oo = feed(off)
        torch.cuda.synchronize()
        for ref, others in ((0, (1, 2)), (3, (4,))):
            for i in others:
                for name in ("params", "grads", "mom", "bn"):
                    assert torch.equal(getattr(nets[ref], name), getattr(nets[i], name)), (name, step, i)
                assert torch.equal(outs[ref]["loss_parts"], outs[i]["loss_parts"]) and torch.equal(outs[ref]["conf"], outs[i]["conf"])
                assert torch.equal(nets[ref].logits[:n], nets[i].logits[:n])
                assert torch.equal(nets[ref].region_grad[:n], nets[i].region_grad[:n]) and torch.equal(nets[ref].lovasz_err[:n], nets[i].lovasz_err[:n])
                assert torch.equal(nets[ref].lovasz_loss[:B], nets[i].lovasz_loss[:B])
        assert not torch.equal(outs[3]["loss_parts"][:1], oo["loss_parts"][:1]) and not torch.equal(nets[3].grads, off.grads)
        assert not torch.equal(nets[0].grads, nets[3].grads)


def test_lambda_zero_or_never_set_leaves_a_training_trajectory_bitwise_unchanged():
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    a, b, c, e = mk(), mk(), mk(), mk(engine=False)
    b.set_lovasz(0)
    e.set_lovasz(0.0)
    c.set_lovasz(LOV)
    assert type(a).__name__ == "EngineNet" and a.lovasz is None and b.lovasz is None and e.lovasz is None and c.lovasz == LOV
    names = ("lovasz_err", "region_grad", "lovasz_loss", "lovasz_scratch")
    for d in (a, b, e):
        for nm in names:
            getattr(d, nm).fill_(MARK)
    for step in range(3):
        x, y, valid = _step_inputs(ch, K, B, S, 30 + step)
        xs, ys = x.reshape(B, -1), y.reshape(B, -1)
        oa, ob, oc, oe = _feed_step(a, xs, ys, S), _feed_step(b, xs, ys, S), _feed_step(c, xs, ys, S), _feed_step(e, xs, ys, S)
        torch.cuda.synchronize()
        for other, oo in ((b, ob), (e, oe)):
            for name in ("params", "mom", "grads", "bn"):
                assert torch.equal(getattr(a, name), getattr(other, name)), (name, step)
            assert torch.equal(oa["loss_parts"], oo["loss_parts"]) and torch.equal(oa["conf"], oo["conf"])
        for d in (a, b, e):
            for nm in names:
                assert (getattr(d, nm) == MARK).all(), nm          # off: no launch touches the buffers
        assert not torch.equal(a.grads, c.grads) and not torch.equal(oa["loss_parts"][:1], oc["loss_parts"][:1])


def test_dice_alone_keeps_the_dice_path(lib):
    """the Dice term on and the Lovasz term off: the engine's step equals the op-level mirror, which calls drs_classifier_loss_dice"""
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    a, e = mk(), mk(engine=False)
    calls = []
    real = lib.call
    for d in (a, e):
        d.set_dice(DICE)
        d.set_lovasz(0)
        d.region_grad.fill_(MARK)
    x, y, valid = _step_inputs(ch, K, B, S, 40)
    oa = _feed_step(a, x.reshape(B, -1), y.reshape(B, -1), S)
    lib.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
    try:
        oe = _feed_step(e, x.reshape(B, -1), y.reshape(B, -1), S)
    finally:
        lib.call = real
    torch.cuda.synchronize()
    assert "drs_classifier_loss_dice" in calls and "drs_classifier_loss_region" not in calls and "drs_patch_lovasz_grad" not in calls
    for name in ("params", "mom", "grads", "bn"):
        assert torch.equal(getattr(a, name), getattr(e, name)), name
    assert torch.equal(oa["loss_parts"], oe["loss_parts"]) and (a.region_grad == MARK).all() and (e.region_grad == MARK).all()


def test_bad_values_are_rejected_by_both_nets():
    from drs_amd.net import DilatedNet
    nets = [DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV), DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV, engine=False)]
    for d in nets:
        for bad in (-1, 65, float("nan"), float("inf"), (1, 0.5), "2", True):
            with pytest.raises(ValueError):
                d.set_lovasz(bad)
        assert d.lovasz is None
        d.set_lovasz(0.1)
        assert d.lovasz == 0.1
        d.set_lovasz(None)
        assert d.lovasz is None


# ------------------------------------------------------------------------------------------------- two ranks
# The spawn pattern and the bounds of tests/test_gpu_dice_loss.py::test_two_rank_step_follows_the_single_rank_step (those of
# tests/test_gpu_dp.py: loss 1e-6 ABSOLUTE, gradients 2e-3, parameters 1e-4), on that test's inputs.
DP = ("dilated8_grsl", 5, 6, 4, 21)
DP_LOV = 0.5


def _dp_inputs():
    from test_gpu_dp import _inputs as dp_inputs
    return dp_inputs()


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import loops
    from drs_amd.dist import TorchComm, shard_slice
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    x, y = _dp_inputs()
    sl = shard_slice(B, rank, world)
    d = DilatedNet(NET, CH, K, 0.005, b_max=B // world, s_max=S, device="cuda:0", seed=3, comm=comm)
    loops.setup_lovasz(d, DP_LOV, comm, lambda *a: None)          # what the loops do: one agree on the bits of lam
    d.feed(x[sl], y[sl], S)
    res = d.train_step(B // world, S, 0.01)
    torch.cuda.synchronize()
    np.savez(out + "_rank%d.npz" % rank, grads=d.grads.cpu().numpy(), params=d.params.cpu().numpy(), bn=d.bn.cpu().numpy(),
             loss=d.loss_value(res["loss_parts"]), conf=res["conf"].cpu().numpy(), lam=np.asarray(d.lovasz))
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_step_follows_the_single_rank_step(tmp_path):
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    out = str(tmp_path) + "/dp"
    mp.spawn(_dp_worker, args=(2, 31800 + os.getpid() % 1000, out), nprocs=2, join=True)
    x, y = _dp_inputs()
    losses = {}
    for lam in (None, DP_LOV):                # (the step without the term too, to show below that it mattered)
        d = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=3)
        d.set_lovasz(lam)
        d.feed(x, y, S)
        res = d.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        losses[lam] = d.loss_value(res["loss_parts"])
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    assert float(r0["lam"]) == float(r1["lam"]) == DP_LOV
    loss = losses[DP_LOV]
    print("two ranks: loss %.9g (rank 0 %.9g), without the Lovasz term %.9g" % (loss, float(r0["loss"]), losses[None]))
    assert abs(loss - losses[None]) > 1e-2 * losses[None]

    def rel(a, b):
        return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))
    print("two ranks: grads %.3g params %.3g bn %.3g" % (rel(r0["grads"], d.grads.cpu().numpy()), rel(r0["params"], d.params.cpu().numpy()),
                                                        rel(r0["bn"], d.bn.cpu().numpy())))
    assert abs(float(r0["loss"]) - loss) < 1e-6
    assert rel(r0["grads"], d.grads.cpu().numpy()) < 2e-3
    assert rel(r0["params"], d.params.cpu().numpy()) < 1e-4
    assert rel(r0["bn"], d.bn.cpu().numpy()) < 1e-6
    np.testing.assert_array_equal(r0["conf"], res["conf"].cpu().numpy())
    np.testing.assert_array_equal(r0["params"], r1["params"])


# ------------------------------------------------------------------------------------------------- loop and command lines
def test_train_loop_prints_the_combined_loss_and_keeps_lambda(tmp_path, capsys, monkeypatch):
    from drs_amd import loops, sampling as SP
    from drs_amd.engine import EngineNet
    from drs_amd.synthetic import make_tile
    from focal_ref import focal_closed_form
    K, WD = 6, 0.005
    tiles = [make_tile(96, 110, 5, K, seed=1, n_seeds=30), make_tile(80, 96, 5, K, seed=2, n_seeds=30)]
    data, labels = [t[0] for t in tiles], [t[1].copy() for t in tiles]
    random.seed(0)
    np.random.seed(0)
    dist = SP.create_distributions_over_classes(labels, 25, 10)
    rot = SP.create_rotation_distribution(dist)
    mean, std = SP.dynamically_calculate_mean_and_std(data, dist, 25)
    seen = []
    step0 = EngineNet.train_step

    def recording(self, B, S, lr0, **kw):
        kw["want_logits"] = True
        out = step0(self, B, S, lr0, **kw)
        M = B * S * S
        seen.append((self.logits[:M * K].cpu().numpy().astype(np.float64).reshape(B, S * S, K), self.labels[:M].cpu().numpy().reshape(B, S * S),
                     out["loss_parts"].cpu().numpy().copy(), self.lovasz_err[:M * K].cpu().numpy().reshape(B, S * S, K)))
        return out
    monkeypatch.setattr(EngineNet, "train_step", recording)
    out = str(tmp_path) + "/"
    net = loops.train(data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 4, WD, mean, std, "loss", "single_fixed",
                      [13], None, None, None, None, 20, out, 1, "dilated_grsl", "vaihingen", "none", device=DEV,
                      val_cache_dir=str(tmp_path), lovasz=1.5)
    text = capsys.readouterr().out
    assert "Lovasz term: lambda 1.5" in text and "Focal loss" not in text and "Dice term" not in text
    assert net.lovasz == 1.5 and net.focal_gamma == 0.0 and net.dice is None
    printed = [float(v) for v in re.findall(r"Training Minibatch: Loss= ([0-9.eE+-]+)", text)]
    assert len(printed) == len(seen) == 4
    for got, (lg, lab, parts, keys) in zip(printed, seen):
        ce = focal_closed_form(lg.reshape(-1, K), lab.reshape(-1).astype(np.int64), np.ones(K), 0.0)["ce"]
        lv = LR.lovasz(lg, lab, K, 1.5, order_keys=keys)
        want = float(ce.mean()) + lv["loss"] + WD * float(parts[1])
        plain = float(ce.mean()) + WD * float(parts[1])
        print("loop loss printed %.6f combined %.6f cross-entropy %.6f" % (got, want, plain))
        assert abs(got - want) < 1e-4 * min(1.0, abs(want)) and abs(plain - want) > 1e-2 * plain
    assert os.path.isfile(out + "lovasz_step_4.npy") and not os.path.exists(out + "dice_step_4.npy")
    assert np.load(out + "lovasz_step_4.npy").tolist() == [1.5]
    # a resumed run trains the same loss and says so; a value given on a resumed run replaces the restored one, and the log says that too
    args = (data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 5, WD, mean, std, "loss", "single_fixed", [13], None, None, None,
            None, 20, out, 1, "dilated_grsl", "vaihingen", out + "model-4")
    net2 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path))
    text = capsys.readouterr().out
    assert "Lovasz term (restored from " + out + "lovasz_step_4.npy): lambda 1.5" in text and net2.lovasz == 1.5
    net3 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path), lovasz=2, focal_gamma=2.0)
    text = capsys.readouterr().out
    assert "Lovasz term: lambda 2" in text and "replacing the value restored from the checkpoint, lambda 1.5" in text
    assert "Focal loss: gamma 2" in text and net3.lovasz == 2.0 and net3.focal_gamma == 2.0


def test_the_three_command_lines_take_the_option(tmp_path, monkeypatch, capsys):
    """one smoke per flavour, at the shapes of tests/test_gpu_loops.py's command-line tests"""
    from drs_amd import cli
    monkeypatch.chdir(tmp_path)           # the reference keeps its .npy caches in the cwd
    out = str(tmp_path) + "/out_"
    random.seed(0)
    np.random.seed(0)
    net = cli.main(["isprs_dilated_random.py", "--lovasz-weight=1.5", "synthetic:70x80x5/vaihingen/", out, "none", "a,b", "c", "0.01", "0.005",
                    "4", "2", "25", "10", "dilated8_grsl", "multi_fixed", "9,13", "acc", "training"], device=DEV)
    assert net.global_step == 2 and net.lovasz == 1.5 and os.path.isfile(out + "lovasz_step_2.npy")
    net = cli.main_coffee(["coffee_dilated_random.py", "synthetic:2x60x60x3/", "synthetic:1x60x60x3/", out, "none", "0.01", "0.001", "6",
                           "2", "25", "10", "dilated_icpr_rate6_small", "multi_fixed", "9,13", "loss", "--lovasz-weight=0.5"], device=DEV)
    assert net.plan.K == 2 and net.global_step == 2 and net.lovasz == 0.5
    net = cli.main_contest(["contest_dilated_random.py", "synthetic:80x70x3/", out, "none", "0.01", "0.001", "4", "2", "25", "10",
                            "dilated_grsl", "multi_fixed", "9,13", "acc", "train", "--lovasz-weight=2", "--dice-weight=1"], device=DEV)
    assert net.plan.K == 7 and net.global_step == 2 and net.lovasz == 2.0 and net.dice == (1.0, 0.5, 0.5, 1.0)
