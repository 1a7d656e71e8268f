"""-m gpu: the soft Dice / Tversky term of the training loss from the kernels up: the coefficient kernel against the
numpy statement (tests/dice_ref.py, itself held against fp64 autograd by tests/test_dice_loss_plan.py), the three forms of the fused
classifier with coefficients against the fp64 closed form, the bitwise no-ops (no coefficients, no labels), a whole training step
against fp64 autograd of the loss written with torch ops, engine = op level, lam = 0, two ranks, the training loop and the three
command lines.

Definition held here: L_dice = inv_n sum_b n_b (lam / K) sum_c (1 - T_bc), T = (TP + eps) / (TP + alpha (SP - TP) + beta (N - TP) + eps)
with the soft counts over the in-loss pixels of patch b alone; it is added to whatever form the cross-entropy has, and class weights,
the focal factor and the pixel map do not weight it.  Tolerances are the project's existing ones: single ops 1e-5 relative to the
tensor's maximum and 1e-6 for the loss, whole nets 1e-4 (logits 1e-3), two ranks as tests/test_gpu_dp.py."""
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import boundary_weight_ref as BR   # noqa: E402
import dice_ref as DR   # noqa: E402
from gpu_util import DEV, dev, rel_err, stream   # noqa: E402
from test_gpu_class_weights import WEIGHTS, _feed_step, _ForcedTorchNet   # noqa: E402  (helpers only)
from test_gpu_focal_loss import FORMS, _check_form, _moderate, _Run   # noqa: E402  (helpers only: the form table, its shared inputs)
from test_gpu_boundary_weight import _blobs, _map, _rotated_corners   # noqa: E402  (helpers only: label blobs, a validity map, a weight map)


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# ------------------------------------------------------------------------------------------------- the coefficient kernel
SHAPES = [(1, 1, 2), (2, 13, 3), (3, 21, 6), (2, 37, 8), (1, 70, 6)]
PARAMS = [(1.0, 0.5, 0.5, 1.0), (2.5, 0.3, 0.7, 0.01)]


def _coef_inputs(B, S, K, seed):
    """name -> (logits float32 [B, S S, K], labels uint8 [B, S S], loss mask uint8 [B, S S] or None).  "mixed": a loss mask with holes,
    labels >= K, class K - 1 absent from patch 0, and (B > 1) a last patch with no pixel in the loss; "no-mask": loss_mask NULL;
    "nothing-in-the-loss": every patch empty"""
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
    return {"mixed": (lg, y, lm), "no-mask": (lg, y, None), "nothing-in-the-loss": (lg, y, np.zeros_like(lm))}


def _coef_launch(lib, lgd, yd, lmd, B, S, K, prm, want_stats=True, guard=0):
    """-> (stats [B, K, 3] or None, coef [B, K, 2], patch_loss [B]) as numpy, plus the raw guarded tensors"""
    g = guard
    stats = torch.full((B * K * 3 + 2 * g,), -7.0, dtype=torch.float64, device=DEV) if want_stats else None
    coef = torch.full((B * K * 2 + 2 * g,), -7.0, dtype=torch.float32, device=DEV)
    pl = torch.full((B + 2 * g,), -7.0, dtype=torch.float64, device=DEV)
    lib.call("drs_patch_dice_coeffs", lgd.data_ptr(), yd.data_ptr(), None if lmd is None else lmd.data_ptr(), B, S, K, *prm,
             None if stats is None else stats[g:].data_ptr(), coef[g:].data_ptr(), pl[g:].data_ptr(), stream())
    torch.cuda.synchronize()
    return stats, coef, pl


def _rel(got, want):
    """largest relative difference; where the reference is exactly zero the value must be too"""
    zero = want == 0
    assert (got[zero] == 0).all()
    return float((np.abs(got - want)[~zero] / np.abs(want[~zero])).max()) if (~zero).any() else 0.0


@pytest.mark.parametrize("B,S,K", SHAPES, ids=["%dx%dx%d-K%d" % (b, s, s, k) for b, s, k in SHAPES])
def test_coefficient_kernel_against_the_reference(lib, B, S, K):
    for name, (lg, y, lm) in _coef_inputs(B, S, K, seed=100 * S + K).items():
        lgd, yd, lmd = dev(lg.reshape(-1)), dev(y.reshape(-1)), None if lm is None else dev(lm.reshape(-1))
        for prm in PARAMS:
            lam, alpha, beta, smooth = prm
            ref = DR.dice(lg.astype(np.float64), y, K, lam, alpha, beta, smooth, loss_mask=lm)       # fp64 on the device's own (fp32) logits
            # the input itself: labels >= K, an absent class, an empty patch where the shape allows it
            if name == "mixed" and S > 1:
                assert (y >= K).any() and ref["cnt"][0, K - 1] == 0 and ref["n"][0] > 0 and (B == 1 or ref["n"][B - 1] == 0)
            if name == "nothing-in-the-loss":
                assert not ref["n"].any()
            stats, coef, pl = _coef_launch(lib, lgd, yd, lmd, B, S, K, prm)
            st = stats.cpu().numpy().reshape(B, K, 3)
            cf = coef.cpu().numpy().reshape(B, K, 2)
            got_pl = pl.cpu().numpy()
            np.testing.assert_array_equal(st[..., 2], ref["cnt"], err_msg=name)                    # N: exact
            # the sums and the patches' loss terms against the reference: the project's tolerance of a loss, 1e-6 relative
            e_tp, e_sp, e_pl = _rel(st[..., 0], ref["tp"]), _rel(st[..., 1], ref["sp"]), _rel(got_pl, ref["patch_loss"])
            print("dice coefficients %dx%dx%d K%d %s %r: TP %.3g SP %.3g patch_loss %.3g" % (B, S, S, K, name, prm, e_tp, e_sp, e_pl))
            assert e_tp < 1e-6 and e_sp < 1e-6 and e_pl < 1e-6, name
            # the coefficients and the patch loss from the device's OWN sums: fp64 evaluation, the coefficients rounded to fp32 once
            own = DR.coefficients(st[..., 0], st[..., 1], st[..., 2], lam, alpha, beta, smooth)
            for got, want in ((cf[..., 0], own["g_in"]), (cf[..., 1], own["g_out"])):
                assert (np.abs(got - want) <= 2.0 ** -23 * np.abs(want) + 1e-45).all(), name
            assert (np.abs(got_pl - own["patch_loss"]) <= 1e-12 * np.abs(own["patch_loss"])).all(), name
            assert (cf[..., 0] <= 0).all() and (cf[..., 1] >= 0).all()
            empty = ref["n"] == 0
            assert not cf[empty].any() and not got_pl[empty].any()                                 # a patch with nothing in the loss: zeros
            # stats_out = NULL gives the same outputs, and a second run the same bits
            _, coef2, pl2 = _coef_launch(lib, lgd, yd, lmd, B, S, K, prm, want_stats=False)
            stats3, coef3, pl3 = _coef_launch(lib, lgd, yd, lmd, B, S, K, prm)
            assert torch.equal(coef, coef2) and torch.equal(pl, pl2)
            assert torch.equal(coef, coef3) and torch.equal(pl, pl3) and torch.equal(stats, stats3)


def test_coefficient_kernel_does_not_write_past_its_patches(lib):
    B, S, K = 3, 21, 6
    lg, y, lm = _coef_inputs(B, S, K, seed=5)["mixed"]
    g = 64
    stats, coef, pl = _coef_launch(lib, dev(lg.reshape(-1)), dev(y.reshape(-1)), dev(lm.reshape(-1)), B, S, K, PARAMS[0], guard=g)
    for t, n in ((stats, B * K * 3), (coef, B * K * 2), (pl, B)):
        assert (t[:g] == -7).all() and (t[g + n:] == -7).all() and (t[g:g + n] != -7).all()


def test_dice_loss_add(lib):
    rng = np.random.default_rng(0)
    for n in (1, 3, 700):
        v = rng.random(n)
        acc = torch.full((3,), 2.5, dtype=torch.float64, device=DEV)
        lib.call("drs_dice_loss_add", dev(v).data_ptr(), n, acc[1:].data_ptr(), stream())
        torch.cuda.synchronize()
        got = acc.cpu().numpy()
        assert got[0] == 2.5 and got[2] == 2.5 and abs(got[1] - (2.5 + v.sum())) < 1e-12 * (2.5 + v.sum())


# ------------------------------------------------------------------------------------------------- the classifier with coefficients
MODES = {"dice-alone": (False, 0.0, False), "on-weights-focal-map": (True, 2.0, True)}
AB = [(0.5, 0.5), (0.3, 0.7)]
LAM, SMOOTH = 1.0, 1.0


class _Dc(object):
    """one launch of drs_classifier_loss_dice and its slab reductions; the fields of test_gpu_focal_loss._Run"""

    RAW = _Run.RAW

    def __init__(self, lib, d, form, wc, gamma, pw, coef, entry="drs_classifier_loss_dice", labels=True):
        C, K, B, S, P = FORMS[form]
        M = B * S * S
        rows = lib.query("drs_classifier_rows", B, S)
        self.logits = torch.zeros(M * K, dtype=torch.float32, device=DEV)
        self.pred = torch.zeros(M, dtype=torch.uint8, device=DEV)
        self.gfeat = torch.zeros(M * C, dtype=torch.float32, device=DEV)
        self.dwp = torch.zeros(rows * C * K, dtype=torch.float32, device=DEV)
        self.dbp = torch.zeros(rows * K, dtype=torch.float32, device=DEV)
        self.lp = torch.zeros(rows, dtype=torch.float64, device=DEV)
        self.conf = torch.zeros(K * K, dtype=torch.int32, device=DEV)
        self.wc = None if wc is None else np.ascontiguousarray(wc, dtype=np.float32)
        head = (d["fd"].data_ptr(), B, S, P, C, 0, C, K, d["wdev"].data_ptr(), d["bdev"].data_ptr(), d["yd"].data_ptr() if labels else None,
                d["lmd"].data_ptr(), d["amd"].data_ptr(), 1.0 / d["n"], None if wc is None else self.wc.ctypes.data, float(gamma),
                None if pw is None else pw.data_ptr())
        mid = {"drs_classifier_loss_dice": (None if coef is None else coef.data_ptr(),), "drs_classifier_loss_pixel": ()}[entry]
        tail = (self.logits.data_ptr(), self.pred.data_ptr(), self.gfeat.data_ptr() if labels else None, C, 0,
                self.dwp.data_ptr() if labels else None, self.dbp.data_ptr() if labels else None, self.lp.data_ptr() if labels else None,
                self.conf.data_ptr() if labels else None, stream())
        lib.call(entry, *(head + mid + tail))
        self.dw = torch.zeros(C * K, dtype=torch.float32, device=DEV)
        self.db = torch.zeros(K, dtype=torch.float32, device=DEV)
        self.ls = torch.zeros(1, dtype=torch.float64, device=DEV)
        if labels:
            scr = torch.zeros(lib.query("drs_colsum_scratch_doubles", C * K), dtype=torch.float64, device=DEV)
            lib.call("drs_rows_reduce_f32", self.dwp.data_ptr(), rows, C * K, self.dw.data_ptr(), scr.data_ptr(), stream())
            lib.call("drs_rows_reduce_f32", self.dbp.data_ptr(), rows, K, self.db.data_ptr(), scr.data_ptr(), stream())
            lib.call("drs_sum_f64", self.lp.data_ptr(), rows, self.ls.data_ptr(), stream())
        torch.cuda.synchronize()


def _coefficients_of(lib, d, form, alpha, beta):
    """the step's pre-pass on the form's inputs: the coefficient kernel on the logits of the plain launch"""
    C, K, B, S, P = FORMS[form]
    coef = torch.zeros(B * K * 2, dtype=torch.float32, device=DEV)
    pl = torch.zeros(B, dtype=torch.float64, device=DEV)
    lib.call("drs_patch_dice_coeffs", d["plain"].logits.data_ptr(), d["yd"].data_ptr(), d["lmd"].data_ptr(), B, S, K, LAM, alpha, beta, SMOOTH,
             None, coef.data_ptr(), pl.data_ptr(), stream())
    torch.cuda.synchronize()
    return coef, pl


def _mode(form, mode):
    C, K, B, S, P = FORMS[form]
    weights, gamma, with_map = MODES[mode]
    return (np.asarray(WEIGHTS[K], dtype=np.float32) if weights else None), gamma, (_map(form) if with_map else None)


CASES = [(f, m, ab) for f in FORMS for m in MODES for ab in AB]


@pytest.mark.parametrize("form,mode,ab", CASES, ids=["%s-%s-a%g-b%g" % (f, m, ab[0], ab[1]) for f, m, ab in CASES])
def test_dice_classifier_against_fp64_numpy(lib, form, mode, ab):
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    d = _moderate(form)
    wc, gamma, pw = _mode(form, mode)
    alpha, beta = ab
    yy, inl = d["yy"], d["inl"]
    # the reference first, all of it from the fp64 logits: the cross-entropy part in its active form, and the Dice term on top
    wc64 = np.ones(K) if wc is None else wc.astype(np.float64)
    pw64 = np.ones(M) if pw is None else pw.astype(np.float64)
    ce = BR.pixel_weighted_closed_form(d["lg_ref"], np.minimum(yy, K - 1), wc64, gamma, pw64)
    ce_loss = float((ce["term"] * inl).sum() / d["n"])
    gl_ce = ce["grad"] * (inl / d["n"])[:, None]
    lm = d["lmd"].cpu().numpy().reshape(B, S * S)
    dc = DR.dice(d["lg_ref"].reshape(B, S * S, K), yy.reshape(B, S * S), K, LAM, alpha, beta, SMOOTH, loss_mask=lm, inv_n=1.0 / d["n"])
    np.testing.assert_array_equal(dc["inl"].reshape(-1), inl)
    gl_dice = dc["grad"].reshape(M, K)
    gl = gl_ce + gl_dice
    w64, f64 = d["w64"], d["f64"]
    gf_ce, gf = gl_ce @ w64.T, gl @ w64.T
    share = float(np.linalg.norm(gf - gf_ce) / np.linalg.norm(gf_ce))
    assert share > 1e-2, share                          # the Dice term changes gfeat by more than 1 % in norm
    coef, pl = _coefficients_of(lib, d, form, alpha, beta)
    r = _Dc(lib, d, form, wc, gamma, None if pw is None else dev(pw), coef)
    plain = d["plain"]
    # untouched: logits, arg-max, confusion matrix -- bit for bit those of drs_classifier_loss
    assert torch.equal(r.logits, plain.logits) and torch.equal(r.pred, plain.pred) and torch.equal(r.conf, plain.conf)
    figures = dict(ce_loss=abs(r.ls.item() / d["n"] - ce_loss) / abs(ce_loss),
                   loss=abs((r.ls.item() + pl.sum().item()) / d["n"] - (ce_loss + dc["loss"])) / abs(ce_loss + dc["loss"]),
                   dice_loss=abs(pl.sum().item() / d["n"] - dc["loss"]) / abs(dc["loss"]),
                   gfeat=rel_err(r.gfeat.cpu().numpy().reshape(M, C), gf), dw=rel_err(r.dw.cpu().numpy().reshape(C, K), f64.T @ gl),
                   db=rel_err(r.db.cpu().numpy(), gl.sum(axis=0)), share=share)
    print("dice classifier %s %s alpha=%g beta=%g: %s" % (form, mode, alpha, beta, figures))
    assert not r.gfeat.view(M, C)[torch.from_numpy(~inl).to(DEV)].any()          # not in the loss: exact zeros
    assert np.isfinite(r.gfeat.cpu().numpy()).all()
    assert figures["ce_loss"] < 1e-6 and figures["loss"] < 1e-6          # loss_partial stays the cross-entropy sum; the step adds the patches' terms
    assert figures["dice_loss"] < 1e-6                                   # ... and the Dice part on its own: no hiding behind the larger part
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5


@pytest.mark.parametrize("form", list(FORMS))
def test_no_coefficients_and_no_labels_are_bitwise_the_pixel_call(lib, form):
    _check_form(form)
    d = _moderate(form)
    coef, _ = _coefficients_of(lib, d, form, 0.5, 0.5)
    for mode in MODES:
        wc, gamma, pw = _mode(form, mode)
        pwd = None if pw is None else dev(pw)
        base = _Dc(lib, d, form, wc, gamma, pwd, None, entry="drs_classifier_loss_pixel")
        assert float(base.gfeat.abs().max()) > 0 and float(base.ls.item()) > 0
        r = _Dc(lib, d, form, wc, gamma, pwd, None)
        for name in _Dc.RAW + ("dw", "db", "ls"):
            assert torch.equal(getattr(r, name), getattr(base, name)), (name, mode)
        # coefficients change the gradients; the cross-entropy sum, the logits, the arg-max and the confusion matrix keep their bits
        r = _Dc(lib, d, form, wc, gamma, pwd, coef)
        assert not torch.equal(r.gfeat, base.gfeat) and not torch.equal(r.dw, base.dw)
        for name in ("logits", "pred", "conf", "lp", "ls"):
            assert torch.equal(getattr(r, name), getattr(base, name)), (name, mode)
        # labels == NULL is an inference launch: the coefficients are not read
        a = _Dc(lib, d, form, wc, gamma, pwd, coef, labels=False)
        b = _Dc(lib, d, form, wc, gamma, pwd, None, entry="drs_classifier_loss_pixel", labels=False)
        assert torch.equal(a.logits, b.logits) and torch.equal(a.pred, b.pred) and torch.equal(a.logits, d["plain"].logits)


# ------------------------------------------------------------------------------------------------- the step
DICE = (1.0, 0.3, 0.7, 1.0)
BW = (10.0, 3.0, 9)
STEP_CASES = [("dilated_grsl", 5, 6, 3, 19), ("dilated_icpr_rate6_densely", 4, 2, 2, 21)]


def _step_inputs(ch, K, B, S, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, S, S, ch)).astype(np.float32)
    y = _blobs(rng, B, S, K).astype(np.int64)
    valid = _rotated_corners(B, S)
    y[valid == 0] = 0
    return x, y, valid


def _torch_dice(logits, y, K, dice, n_glob):
    """L_dice written with torch ops, patch by patch (every pixel in the loss): not the closed form"""
    lam, alpha, beta, smooth = dice
    B = logits.shape[0]
    total = 0.0
    for b in range(B):
        p = torch.softmax(logits[b].reshape(-1, K), dim=1)
        oh = torch.nn.functional.one_hot(torch.as_tensor(y[b].reshape(-1), dtype=torch.long), K).to(p.dtype)
        tp, fp, fn = (p * oh).sum(dim=0), (p * (1.0 - oh)).sum(dim=0), ((1.0 - p) * oh).sum(dim=0)
        total = total + p.shape[0] * (lam / K) * (1.0 - (tp + smooth) / (tp + alpha * fp + beta * fn + smooth)).sum()
    return total / n_glob


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES, ids=["Dilated6Pooling", "DenseDilated6"])
def test_dice_step_against_fp64_autograd(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    WD, GAMMA = 0.005, 2.0
    d = DilatedNet(net, ch, K, WD, b_max=B, s_max=S, device=DEV, seed=11)
    x, y, valid = _step_inputs(ch, K, B, S, 11)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32) + 0.25
    d.set_class_weights(wc)                 # on top of class weights, the focal factor and the boundary weight
    d.set_focal_gamma(GAMMA)
    d.set_boundary_weight(BW)
    d.set_dice(DICE)
    assert d.dice == DICE and d.boundary_weight == BW
    pw_ref, _ = BR.boundary_weight(y.astype(np.uint8), valid, BW[2], BW[0], 1.0 / (2.0 * BW[1] ** 2))
    params = {n: d.get_variable(n).astype(np.float64) for n in d.variable_names()}
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S, acc_mask=valid.reshape(B, -1))
    out = d.train_step(B, S, 0.01, apply_update=False, want_logits=True)
    torch.cuda.synchronize()
    M = B * S * S
    dec = []
    for i, L in enumerate(d.plan.layers):
        z = d.z[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        mr = d.mean_rstd[i].cpu().numpy().reshape(L.cout, 2)
        dcs = {"pos": (z - mr[:, 0]) * mr[:, 1] > 0}
        if d._is_max(i):
            dcs["idx"] = d.idx[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        dec.append(dcs)

    def total(tn):
        """the loss written with torch ops: the weighted focal cross-entropy with the reference's map, plus the Dice term"""
        for q in tn.params_list():
            q.grad = None
        logits = tn.forward(x.astype(np.float64), True)
        yy = torch.as_tensor(y.reshape(-1), dtype=torch.long)
        logp = torch.log_softmax(logits.reshape(-1, K), dim=1).gather(1, yy[:, None])[:, 0]
        l2 = sum(0.5 * (w_ ** 2).sum() for w_ in list(tn.w.values()) + list(tn.fcw.values()))
        pw = torch.as_tensor(pw_ref.reshape(-1), dtype=torch.float64)
        ce = (pw * torch.as_tensor(wc, dtype=torch.float64)[yy] * (1.0 - torch.exp(logp)) ** GAMMA * (-logp)).sum() / M
        lg_nhwc = logits if logits.shape[-1] == K else logits.permute(0, 2, 3, 1)
        dice = _torch_dice(lg_nhwc, y, K, DICE, M)
        loss = ce + dice + WD * l2
        loss.backward()
        return float(loss.detach()), logits.detach().numpy(), float((ce + WD * l2).detach())
    forced = _ForcedTorchNet(net, ch, K, params=params, dtype=torch.float64)
    forced.dec = dec
    loss_ref, logits_ref, loss_without = total(forced)
    got_loss = d.loss_value(out["loss_parts"])
    print("dice step %s: loss %.9g forced %.9g (without the Dice term %.9g)" % (net, got_loss, loss_ref, loss_without))
    assert abs(loss_ref - loss_without) > 1e-2 * loss_without
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
    # the untouched quantities of the same step: the confusion matrix counts the valid pixels, each once
    cm = np.zeros((K, K), dtype=np.int64)
    ok = valid.reshape(-1) != 0
    np.add.at(cm, (y.reshape(-1)[ok], out["pred"].cpu().numpy().reshape(-1)[ok]), 1)
    np.testing.assert_array_equal(out["conf"].cpu().numpy().reshape(K, K), cm)
    # an eval forward ignores the option
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S)
    _, l1 = d.forward(B, S)
    l1 = l1.clone()
    d.set_dice(None)
    _, l0 = d.forward(B, S)
    assert torch.equal(l0, l1)


def test_dice_step_with_a_loss_mask_counts_patches_by_their_valid_pixels():
    """contest's void mask: the step's Dice term against the numpy statement on the step's own logits, global_pixels = the unmasked count"""
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    d = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=5)
    x, y, _ = _step_inputs(ch, K, B, S, 5)
    rng = np.random.default_rng(5)
    mask = (rng.random((B, S * S)) < 0.6).astype(np.uint8)
    mask[1] = 0                                       # a patch that is all void
    n = int(mask.sum())
    losses = {}
    for dice in (None, DICE):
        d.set_dice(dice)
        d.feed(x.reshape(B, -1), y.reshape(B, -1), S, mask=mask)
        out = d.train_step(B, S, 0.01, use_loss_mask=True, global_pixels=n, apply_update=False, want_logits=True)
        torch.cuda.synchronize()
        losses[dice] = float(out["loss_parts"][0].item())
    lg = d.logits[:B * S * S * K].cpu().numpy().astype(np.float64).reshape(B, S * S, K)
    ref = DR.dice(lg, y.reshape(B, -1), K, *DICE, loss_mask=mask, inv_n=1.0 / n)
    assert ref["n"][1] == 0 and ref["patch_loss"][1] == 0 and ref["loss"] > 1e-2 * losses[None]
    print("dice step with a loss mask: %.9g = %.9g + %.9g" % (losses[DICE], losses[None], ref["loss"]))
    assert abs(losses[DICE] - losses[None] - ref["loss"]) < 1e-6 * losses[DICE]


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES)
def test_step_engine_equals_op_level_and_repeats_bitwise(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    from drs_amd.engine import EngineNet
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    nets = [mk(), mk(engine=False), mk(), mk(), mk(engine=False)]
    assert isinstance(nets[0], EngineNet) and not isinstance(nets[1], EngineNet)
    for d in nets[:3]:                       # on top of class weights, the focal term and the boundary weight ...
        d.set_class_weights(WEIGHTS[K])
        d.set_focal_gamma(2.0)
        d.set_boundary_weight(BW)
    for d in nets:                           # ... and alone
        d.set_dice(DICE)
        assert d.dice == DICE
    off = mk()
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
                assert torch.equal(nets[ref].logits[:B * S * S * K], nets[i].logits[:B * S * S * K])
                assert torch.equal(nets[ref].dice_coef[:B * K * 2], nets[i].dice_coef[:B * K * 2])
                assert torch.equal(nets[ref].dice_loss[:B], nets[i].dice_loss[:B])
        assert not torch.equal(outs[3]["loss_parts"][:1], oo["loss_parts"][:1]) and not torch.equal(nets[3].grads, off.grads)
        assert not torch.equal(nets[0].grads, nets[3].grads)


def test_lambda_zero_or_never_set_leaves_a_training_trajectory_bitwise_unchanged():
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    a, b, c, e = mk(), mk(), mk(), mk(engine=False)
    b.set_dice((0, 0.3, 0.7, 2))
    e.set_dice(0)
    c.set_dice(DICE)
    assert type(a).__name__ == "EngineNet" and a.dice is None and b.dice is None and e.dice is None and c.dice == DICE
    mark_c, mark_l = torch.full_like(a.dice_coef, -7.0), torch.full_like(a.dice_loss, -7.0)
    for d in (a, b, e):
        d.dice_coef.copy_(mark_c)
        d.dice_loss.copy_(mark_l)
    for step in range(3):
        x, y, valid = _step_inputs(ch, K, B, S, 30 + step)
        xs, ys = x.reshape(B, -1), y.reshape(B, -1)
        oa, ob, oc, oe = _feed_step(a, xs, ys, S), _feed_step(b, xs, ys, S), _feed_step(c, xs, ys, S), _feed_step(e, xs, ys, S)
        torch.cuda.synchronize()
        for other, oo in ((b, ob), (e, oe)):
            for name in ("params", "mom", "grads", "bn"):
                assert torch.equal(getattr(a, name), getattr(other, name)), (name, step)
            assert torch.equal(oa["loss_parts"], oo["loss_parts"]) and torch.equal(oa["conf"], oo["conf"])
            assert torch.equal(other.dice_coef, mark_c) and torch.equal(other.dice_loss, mark_l)          # off: no launch touches the buffers
        assert not torch.equal(a.grads, c.grads) and not torch.equal(oa["loss_parts"][:1], oc["loss_parts"][:1])


def test_bad_quadruples_are_rejected_by_both_nets():
    from drs_amd.net import DilatedNet
    nets = [DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV), DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV, engine=False)]
    for d in nets:
        for bad in (-1, 65, float("nan"), (1, 0.5), (1, 2, 0.5), (1, 0.5, 0.5, 0), "2", (1, 2, 3, 4, 5)):
            with pytest.raises(ValueError):
                d.set_dice(bad)
        assert d.dice is None
        d.set_dice((0.1, 0.3, 0.7))
        assert d.dice == (0.1, 0.3, 0.7, 1.0)
        d.set_dice(None)
        assert d.dice is None


# ------------------------------------------------------------------------------------------------- two ranks
# The spawn pattern and the bounds of test_gpu_boundary_weight.py::test_two_rank_step_follows_the_single_rank_step (those of
# tests/test_gpu_dp.py::test_two_rank_step_equals_single_rank: loss 1e-6 ABSOLUTE, gradients 2e-3, parameters 1e-4), on that test's
# inputs.  The per-patch definition is what this test exists for: each rank sums over its own patches only, and the all-reduce of
# the loss scalar keeps its count of 1.
DP = ("dilated8_grsl", 5, 6, 4, 21)
DP_DICE = (0.5, 0.5, 0.5, 1.0)


def _dp_inputs():
    from test_gpu_dp import _inputs
    return _inputs()


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
    loops.setup_dice(d, DP_DICE, comm, lambda *a: None)          # what the loops do: one agree on the quadruple's bits
    d.feed(x[sl], y[sl], S)
    res = d.train_step(B // world, S, 0.01)
    torch.cuda.synchronize()
    np.savez(out + "_rank%d.npz" % rank, grads=d.grads.cpu().numpy(), params=d.params.cpu().numpy(), bn=d.bn.cpu().numpy(),
             loss=d.loss_value(res["loss_parts"]), conf=res["conf"].cpu().numpy(), dice=np.asarray(d.dice))
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_step_follows_the_single_rank_step(tmp_path):
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    out = str(tmp_path) + "/dp"
    mp.spawn(_dp_worker, args=(2, 30800 + os.getpid() % 1000, out), nprocs=2, join=True)
    x, y = _dp_inputs()
    losses = {}
    for dice in (None, DP_DICE):                # (the step without the term too, to show below that it mattered)
        d = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=3)
        d.set_dice(dice)
        d.feed(x, y, S)
        res = d.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        losses[dice] = d.loss_value(res["loss_parts"])
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    assert tuple(r0["dice"]) == tuple(r1["dice"]) == DP_DICE
    loss = losses[DP_DICE]
    print("two ranks: loss %.9g (rank 0 %.9g), without the Dice term %.9g" % (loss, float(r0["loss"]), losses[None]))
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
def test_train_loop_prints_the_combined_loss_and_keeps_the_quadruple(tmp_path, capsys, monkeypatch):
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
                     out["loss_parts"].cpu().numpy().copy()))
        return out
    monkeypatch.setattr(EngineNet, "train_step", recording)
    out = str(tmp_path) + "/"
    net = loops.train(data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 4, WD, mean, std, "loss", "single_fixed",
                      [13], None, None, None, None, 20, out, 1, "dilated_grsl", "vaihingen", "none", device=DEV,
                      val_cache_dir=str(tmp_path), dice=(1, 0.3, 0.7))
    text = capsys.readouterr().out
    assert "Dice term: lambda 1 alpha 0.3 beta 0.7 smooth 1" in text and "Focal loss" not in text and "Boundary weight" not in text
    assert net.dice == (1.0, 0.3, 0.7, 1.0) and net.focal_gamma == 0.0 and net.boundary_weight is None
    printed = [float(v) for v in re.findall(r"Training Minibatch: Loss= ([0-9.eE+-]+)", text)]
    assert len(printed) == len(seen) == 4
    for got, (lg, lab, parts) in zip(printed, seen):
        ce = focal_closed_form(lg.reshape(-1, K), lab.reshape(-1).astype(np.int64), np.ones(K), 0.0)["ce"]
        dc = DR.dice(lg, lab, K, 1.0, 0.3, 0.7, 1.0)
        want = float(ce.mean()) + dc["loss"] + WD * float(parts[1])
        plain = float(ce.mean()) + WD * float(parts[1])
        print("loop loss printed %.6f combined %.6f cross-entropy %.6f" % (got, want, plain))
        assert abs(got - want) < 1e-4 * min(1.0, abs(want)) and abs(plain - want) > 1e-2 * plain
    assert os.path.isfile(out + "dice_step_4.npy") and not os.path.exists(out + "focal_gamma_step_4.npy")
    assert np.load(out + "dice_step_4.npy").tolist() == [1.0, 0.3, 0.7, 1.0]
    # a resumed run trains the same loss and says so; a quadruple given on a resumed run replaces the restored one, and the log says that too
    args = (data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 5, WD, mean, std, "loss", "single_fixed", [13], None, None, None,
            None, 20, out, 1, "dilated_grsl", "vaihingen", out + "model-4")
    net2 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path))
    text = capsys.readouterr().out
    assert "Dice term (restored from " + out + "dice_step_4.npy): lambda 1 alpha 0.3 beta 0.7 smooth 1" in text and net2.dice == (1.0, 0.3, 0.7, 1.0)
    net3 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path), dice=2, focal_gamma=2.0)
    text = capsys.readouterr().out
    assert "Dice term: lambda 2 alpha 0.5 beta 0.5 smooth 1" in text
    assert "replacing the quadruple restored from the checkpoint, lambda 1 alpha 0.3 beta 0.7 smooth 1" in text
    assert "Focal loss: gamma 2" in text and net3.dice == (2.0, 0.5, 0.5, 1.0) and net3.focal_gamma == 2.0


def test_the_three_command_lines_take_the_option(tmp_path, monkeypatch, capsys):
    """one smoke per flavour, at the shapes of tests/test_gpu_loops.py's command-line tests"""
    from drs_amd import cli
    monkeypatch.chdir(tmp_path)           # the reference keeps its .npy caches in the cwd
    out = str(tmp_path) + "/out_"
    random.seed(0)
    np.random.seed(0)
    net = cli.main(["isprs_dilated_random.py", "--dice-weight=1,0.3,0.7", "synthetic:70x80x5/vaihingen/", out, "none", "a,b", "c", "0.01", "0.005",
                    "4", "2", "25", "10", "dilated8_grsl", "multi_fixed", "9,13", "acc", "training"], device=DEV)
    assert net.global_step == 2 and net.dice == (1.0, 0.3, 0.7, 1.0) and os.path.isfile(out + "dice_step_2.npy")
    net = cli.main_coffee(["coffee_dilated_random.py", "synthetic:2x60x60x3/", "synthetic:1x60x60x3/", out, "none", "0.01", "0.001", "6",
                           "2", "25", "10", "dilated_icpr_rate6_small", "multi_fixed", "9,13", "loss", "--dice-weight=0.5"], device=DEV)
    assert net.plan.K == 2 and net.global_step == 2 and net.dice == (0.5, 0.5, 0.5, 1.0)
    net = cli.main_contest(["contest_dilated_random.py", "synthetic:80x70x3/", out, "none", "0.01", "0.001", "4", "2", "25", "10",
                            "dilated_grsl", "multi_fixed", "9,13", "acc", "train", "--dice-weight=2,0.5,0.5,0.1"], device=DEV)
    assert net.plan.K == 7 and net.global_step == 2 and net.dice == (2.0, 0.5, 0.5, 0.1)
    assert capsys.readouterr().out.count("Dice term: lambda") == 3
