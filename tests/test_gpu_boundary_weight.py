"""-m gpu: the boundary-weighted training loss from the kernels up: the weight-map kernel against the numpy statement
(tests/boundary_weight_ref.py: distances exact, weights within one fp32 ulp of the fp64 value), the three forms of the fused classifier
with a map against the fp64 closed form, the bitwise no-ops (no map, a map of ones), a 0/1 map against the same pattern as loss mask,
a whole training step against fp64 autograd with the reference's map, engine = op level, two ranks, and the training loop.

Definition held here: L = inv_n * sum over the pixels in the loss of pw[p] wc[y] m CE with pw = 1 + a exp(-D2 c), D2 the squared
distance to the nearest valid pixel of another byte inside the patch and the (2R + 1)^2 window (pw = 1 where there is none or the
pixel is invalid); inv_n stays 1 / the number of pixels the loss averages over.  Tolerances are the project's existing ones: single ops
1e-5 relative to the tensor's maximum and 1e-6 for the loss, whole nets 1e-4, two ranks as tests/test_gpu_dp.py."""
import functools
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import boundary_weight_ref as BR   # noqa: E402
from gpu_util import DEV, dev, rel_err, stream   # noqa: E402
from test_gpu_class_weights import WEIGHTS, _feed_step, _ForcedTorchNet   # noqa: E402  (helpers only)
from test_gpu_focal_loss import FORMS, _check_form, _figures, _moderate, _Run   # noqa: E402  (helpers only: the form table, its shared inputs)


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# ------------------------------------------------------------------------------------------------- inputs of the weight kernel
SHAPES = [(1, 1, 1), (2, 13, 1), (3, 9, 16), (3, 21, 4), (2, 33, 16), (2, 37, 8), (1, 70, 16)]


def _blobs(rng, B, S, ncls):
    """a few large regions per patch: nearest of 2 * ncls seeds, classes drawn from [0, ncls)"""
    yy, xx = np.mgrid[0:S, 0:S]
    lab = np.zeros((B, S, S), dtype=np.uint8)
    for b in range(B):
        n = 2 * ncls
        sy, sx = rng.integers(0, S, size=n), rng.integers(0, S, size=n)
        cls = np.concatenate([np.arange(ncls), rng.integers(0, ncls, size=n - ncls)])
        near = np.argmin((yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2, axis=0)
        lab[b] = cls[near]
    return lab


def _rotated_corners(B, S):
    """what a rotated crop leaves: a square turned by 30 degrees about the centre is valid, the corners are not"""
    yy, xx = np.mgrid[0:S, 0:S]
    c = (S - 1) / 2.0
    u = (xx - c) * np.cos(np.pi / 6) + (yy - c) * np.sin(np.pi / 6)
    v = -(xx - c) * np.sin(np.pi / 6) + (yy - c) * np.cos(np.pi / 6)
    ok = (np.abs(u) <= 0.42 * S + 0.5) & (np.abs(v) <= 0.42 * S + 0.5)
    return np.repeat(ok[None].astype(np.uint8), B, axis=0)


def _inputs(B, S, R, seed):
    """name -> (lab, valid or None, uniform): every label and validity input of the issue at one shape.  uniform: True where the
    input can hold no finite distance at all -- uniform patches, a single pixel, a band wider than the window, an only patch that is
    all invalid"""
    rng = np.random.default_rng(seed)
    out = {}
    for ncls in (2, 4, 6):
        out["blobs%d" % ncls] = (_blobs(rng, B, S, ncls), None, False)
    lab = _blobs(rng, B, S, 3)
    lab[lab == 1] = 200                               # a byte >= K is just a byte
    lab[0, S // 2:, :][lab[0, S // 2:, :] == 2] = 255
    out["byte>=K"] = (lab, None, False)
    lab = _blobs(rng, B, S, 5)
    valid = _rotated_corners(B, S)
    lab[valid == 0] = 0                               # the crop kernel's fill under mask 0
    out["rotated-corners"] = (lab, valid, False)
    lab = np.zeros((B, S, S), dtype=np.uint8)
    lab[:, :, S // 2:] = 3
    valid = np.ones((B, S, S), dtype=np.uint8)
    lo, hi = max(0, S // 2 - 1), min(S, S // 2 + 2)
    valid[:, :, lo:hi] = 0
    lab[:, :, lo:hi] = 0
    out["invalid-band"] = (lab, valid, R < hi - lo + 1)          # crossing the band takes hi - lo + 1 columns
    lab = _blobs(rng, B, S, 4)
    valid = (rng.random((B, S, S)) < 0.85).astype(np.uint8)
    valid[B - 1] = 0                                  # an all-invalid patch
    out["all-invalid-patch"] = (lab, valid, B == 1)
    lab = np.zeros((B, S, S), dtype=np.uint8)
    for b in range(B):
        lab[b] = 1 + 2 * b                            # uniform patches with different labels: every weight is 1
    out["uniform-patches"] = (lab, None, True)
    lab = np.zeros((B, S, S), dtype=np.uint8)
    lab[:, 1::2, 0] = 4                               # a row ends in class 0 while the next begins in class 4
    out["row-wrap"] = (lab, None, S == 1)
    return out


def _ulps(a, b):
    """distance in float32 steps between two non-negative float32 arrays"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _launch(lib, labd, vald, B, S, R, a, c, want_d2=True):
    w = torch.full((B, S, S), -7.0, dtype=torch.float32, device=DEV)
    d2 = torch.full((B, S, S), -7, dtype=torch.int16, device=DEV) if want_d2 else None
    lib.call("drs_patch_boundary_weight", labd.data_ptr(), None if vald is None else vald.data_ptr(), B, S, R, float(a), float(c),
             None if d2 is None else d2.data_ptr(), w.data_ptr(), stream())
    torch.cuda.synchronize()
    return w, d2


@pytest.mark.parametrize("B,S,R", SHAPES, ids=["%dx%dx%d-R%d" % (b, s, s, r) for b, s, r in SHAPES])
def test_weight_kernel_against_the_reference(lib, B, S, R):
    sigma = max(1.0, R / 3.0)
    c = 1.0 / (2.0 * sigma * sigma)
    for name, (lab, valid, uniform) in _inputs(B, S, R, seed=100 * S + R).items():
        d2_ref = BR.boundary_d2(lab, valid, R)
        fin = d2_ref != BR.INF
        # the input itself: both kinds of pixel where the shape allows it
        if not uniform and S > 1:
            assert fin.any(), name
        if uniform:
            assert not fin.any(), name
        if (valid is not None and (valid == 0).any()) or S >= 4 * R + 5:
            assert (~fin).any(), name
        labd, vald = dev(lab), None if valid is None else dev(valid)
        for a in (-1.0, 0.5, 10.0):
            w, d2 = _launch(lib, labd, vald, B, S, R, a, c)
            got_d2 = d2.cpu().numpy().view(np.uint16)
            np.testing.assert_array_equal(got_d2, BR.d2_u16(d2_ref), err_msg="%s a=%g" % (name, a))
            w_ref, _ = BR.boundary_weight(lab, valid, R, a, c)
            got = w.cpu().numpy()
            assert (got[~fin] == 1.0).all(), name
            assert (got >= 0).all() and np.isfinite(got).all()
            steps = _ulps(got, w_ref.astype(np.float32))
            assert steps.max() <= 1, (name, a, int(steps.max()))
            if uniform:
                assert (got == 1.0).all()
            # d2_out = NULL gives the same weights, and a second run the same bits
            w2, _ = _launch(lib, labd, vald, B, S, R, a, c, want_d2=False)
            w3, d3 = _launch(lib, labd, vald, B, S, R, a, c)
            assert torch.equal(w, w2) and torch.equal(w, w3) and torch.equal(d2, d3)


def test_weight_kernel_does_not_write_past_its_patches(lib):
    """B S S floats and shorts, nothing beyond: the arrays sit inside larger ones filled with a mark"""
    B, S, R = 3, 21, 4
    lab = _blobs(np.random.default_rng(3), B, S, 4)
    M = B * S * S
    w = torch.full((M + 256,), -7.0, dtype=torch.float32, device=DEV)
    d2 = torch.full((M + 256,), -7, dtype=torch.int16, device=DEV)
    lib.call("drs_patch_boundary_weight", dev(lab).data_ptr(), None, B, S, R, 10.0, 0.125, d2[128:].data_ptr(), w[128:].data_ptr(), stream())
    torch.cuda.synchronize()
    assert (w[:128] == -7).all() and (w[128 + M:] == -7).all() and (d2[:128] == -7).all() and (d2[128 + M:] == -7).all()
    assert (w[128:128 + M] >= 1.0).all()


def test_boundary_weight_map_helper(lib):
    from drs_amd import loops
    B, S = 2, 33
    lab, valid, _ = _inputs(B, S, 12, seed=9)["rotated-corners"]
    w, d2 = loops.boundary_weight_map(lab, valid, 10, 4, 12)
    w_ref, d2_ref = BR.boundary_weight(lab, valid, 12, 10.0, 1.0 / 32.0)
    assert w.shape == d2.shape == (B, S, S) and w.dtype == torch.float32 and d2.dtype == torch.int32
    np.testing.assert_array_equal(d2.cpu().numpy(), BR.d2_u16(d2_ref).astype(np.int32))
    assert _ulps(w.cpu().numpy(), w_ref.astype(np.float32)).max() <= 1
    w2, _ = loops.boundary_weight_map(dev(lab), None, 10, 4, 12)
    assert not torch.equal(w, w2)                     # the validity map matters
    with pytest.raises(ValueError):
        loops.boundary_weight_map(lab, valid, 65, 4, 12)
    with pytest.raises(ValueError):
        loops.boundary_weight_map(lab[0], None, 10, 4, 12)


# ------------------------------------------------------------------------------------------------- the classifier with a map
MODES = {"plain": (False, 0.0), "class-weights": (True, 0.0), "focal-g2": (True, 2.0)}


class _Px(object):
    """one launch of drs_classifier_loss_pixel and its slab reductions; the fields of test_gpu_focal_loss._Run"""

    RAW = _Run.RAW

    def __init__(self, lib, d, form, wc, gamma, pw, lmd="own"):
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
        lmd = d["lmd"] if isinstance(lmd, str) else lmd
        self.wc = None if wc is None else np.ascontiguousarray(wc, dtype=np.float32)
        lib.call("drs_classifier_loss_pixel", d["fd"].data_ptr(), B, S, P, C, 0, C, K, d["wdev"].data_ptr(), d["bdev"].data_ptr(),
                 d["yd"].data_ptr(), None if lmd is None else lmd.data_ptr(), d["amd"].data_ptr(), 1.0 / d["n"],
                 None if wc is None else self.wc.ctypes.data, float(gamma), None if pw is None else pw.data_ptr(), self.logits.data_ptr(),
                 self.pred.data_ptr(), self.gfeat.data_ptr(), C, 0, self.dwp.data_ptr(), self.dbp.data_ptr(), self.lp.data_ptr(),
                 self.conf.data_ptr(), stream())
        self.dw = torch.zeros(C * K, dtype=torch.float32, device=DEV)
        self.db = torch.zeros(K, dtype=torch.float32, device=DEV)
        self.ls = torch.zeros(1, dtype=torch.float64, device=DEV)
        scr = torch.zeros(lib.query("drs_colsum_scratch_doubles", C * K), dtype=torch.float64, device=DEV)
        lib.call("drs_rows_reduce_f32", self.dwp.data_ptr(), rows, C * K, self.dw.data_ptr(), scr.data_ptr(), stream())
        lib.call("drs_rows_reduce_f32", self.dbp.data_ptr(), rows, K, self.db.data_ptr(), scr.data_ptr(), stream())
        lib.call("drs_sum_f64", self.lp.data_ptr(), rows, self.ls.data_ptr(), stream())
        torch.cuda.synchronize()


def _focal_run(lib, d, form, wc, gamma, lmd="own"):
    C, K, B, S, P = FORMS[form]
    return _Run(lib, d["fd"], B, S, P, C, K, d["wdev"], d["bdev"], d["yd"], d["lmd"] if isinstance(lmd, str) else lmd, d["amd"], 1.0 / d["n"],
                wc, gamma)


@functools.lru_cache(maxsize=4)
def _map(form):
    """a weight map of the kind the kernel makes, for the pixels of a form: 1 + 10 exp(-D2 / 32) at random distances, 30 % exactly 1,
    a few zeros (a = -1 at D2 -> 0 is the smallest weight the domain allows)"""
    C, K, B, S, P = FORMS[form]
    rng = np.random.default_rng(B * S + K)
    M = B * S * S
    pw = (1.0 + 10.0 * np.exp(-rng.integers(1, 300, size=M) / 32.0)).astype(np.float32)
    pw[rng.random(M) < 0.3] = 1.0
    pw[rng.random(M) < 0.02] = 0.0
    return pw


def _wc(K, mode):
    return np.asarray(WEIGHTS[K], dtype=np.float32) if MODES[mode][0] else None


CASES = [(f, m) for f in FORMS for m in MODES]


@pytest.mark.parametrize("form,mode", CASES, ids=["%s-%s" % fm for fm in CASES])
def test_pixel_classifier_against_fp64_numpy(lib, form, mode):
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    d = _moderate(form)
    wc, gamma = _wc(K, mode), MODES[mode][1]
    pw = _map(form)
    r = _Px(lib, d, form, wc, gamma, dev(pw))
    plain = d["plain"]
    # not weighted: logits, arg-max, confusion matrix -- bit for bit those of drs_classifier_loss
    assert torch.equal(r.logits, plain.logits) and torch.equal(r.pred, plain.pred) and torch.equal(r.conf, plain.conf)
    yy, inl = d["yy"], d["inl"]
    wc64 = np.ones(K) if wc is None else wc.astype(np.float64)
    ref = BR.pixel_weighted_closed_form(d["lg_ref"], np.minimum(yy, K - 1), wc64, gamma, pw.astype(np.float64))
    loss_ref = float((ref["term"] * inl).sum() / d["n"])
    gl = ref["grad"] * (inl / d["n"])[:, None]
    figures = _figures(r, d, loss_ref, gl, M, C, K)
    print("pixel classifier %s %s: %s" % (form, mode, figures))
    unweighted = float((wc64[np.minimum(yy, K - 1)] * ref["m"] * ref["ce"] * inl).sum() / d["n"])
    assert abs(loss_ref - unweighted) > 1e-2 * unweighted          # the map changes the loss by more than 1 %
    assert not r.gfeat.view(M, C)[torch.from_numpy(~inl | (pw == 0)).to(DEV)].any()      # weight 0 / not in the loss: exact zeros
    assert np.isfinite(r.gfeat.cpu().numpy()).all()
    assert figures["loss"] < 1e-6
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5


@pytest.mark.parametrize("form", list(FORMS))
def test_no_map_and_a_map_of_ones_are_bitwise_the_focal_call(lib, form):
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    d = _moderate(form)
    ones = torch.ones(B * S * S, dtype=torch.float32, device=DEV)
    pwd = dev(_map(form))
    for mode in MODES:
        wc, gamma = _wc(K, mode), MODES[mode][1]
        base = _focal_run(lib, d, form, wc, gamma)
        assert float(base.gfeat.abs().max()) > 0 and float(base.ls.item()) > 0
        for what, pw in (("NULL", None), ("ones", ones)):
            r = _Px(lib, d, form, wc, gamma, pw)
            for name in _Px.RAW + ("dw", "db", "ls"):
                assert torch.equal(getattr(r, name), getattr(base, name)), (name, mode, what)
        # a real map changes the gradients and the loss, not the logits' bits
        r = _Px(lib, d, form, wc, gamma, pwd)
        assert not torch.equal(r.gfeat, base.gfeat) and not torch.equal(r.ls, base.ls)
        assert torch.equal(r.logits, base.logits) and torch.equal(r.pred, base.pred) and torch.equal(r.conf, base.conf)


@pytest.mark.parametrize("form", list(FORMS))
def test_a_zero_one_map_is_the_same_pattern_as_loss_mask(lib, form):
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    d = _moderate(form)
    rng = np.random.default_rng(M + K)
    pat = (rng.random(M) < 0.6).astype(np.uint8)
    lm = d["lmd"].cpu().numpy()
    both = dev(lm & pat)
    for mode in MODES:
        wc, gamma = _wc(K, mode), MODES[mode][1]
        a = _Px(lib, d, form, wc, gamma, dev(pat.astype(np.float32)))
        b = _focal_run(lib, d, form, wc, gamma, lmd=both)
        for name in ("gfeat", "dwp", "dbp", "lp", "dw", "db", "ls"):            # equal as numbers: -0 == 0
            assert bool((getattr(a, name) == getattr(b, name)).all()), (name, mode)
        assert torch.equal(a.logits, b.logits) and torch.equal(a.pred, b.pred) and torch.equal(a.conf, b.conf)
        assert float(a.ls.item()) > 0


def test_no_labels_ignores_the_map(lib):
    """labels == NULL is an inference launch: the map is not read"""
    form = "mfma-K6"
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    d = _moderate(form)
    out = []
    for pw in (None, dev(_map(form))):
        logits = torch.zeros(M * K, dtype=torch.float32, device=DEV)
        pred = torch.zeros(M, dtype=torch.uint8, device=DEV)
        lib.call("drs_classifier_loss_pixel", d["fd"].data_ptr(), B, S, P, C, 0, C, K, d["wdev"].data_ptr(), d["bdev"].data_ptr(), None, None, None,
                 1.0, None, 0.0, None if pw is None else pw.data_ptr(), logits.data_ptr(), pred.data_ptr(), None, 0, 0, None, None, None, None,
                 stream())
        torch.cuda.synchronize()
        out.append((logits, pred))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], d["plain"].logits)


# ------------------------------------------------------------------------------------------------- the step
BW = (10.0, 3.0, 9)
STEP_CASES = [("dilated_grsl", 5, 6, 3, 19), ("dilated_icpr_rate6_densely", 4, 2, 2, 21)]


def _step_inputs(ch, K, B, S, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, S, S, ch)).astype(np.float32)
    y = _blobs(rng, B, S, K).astype(np.int64)
    valid = _rotated_corners(B, S)
    y[valid == 0] = 0
    return x, y, valid


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES, ids=["Dilated6Pooling", "DenseDilated6"])
def test_boundary_weighted_step_against_fp64_autograd(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    WD, GAMMA = 0.005, 2.0
    d = DilatedNet(net, ch, K, WD, b_max=B, s_max=S, device=DEV, seed=11)
    x, y, valid = _step_inputs(ch, K, B, S, 11)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32) + 0.25
    d.set_class_weights(wc)
    d.set_focal_gamma(GAMMA)
    d.set_boundary_weight(BW)
    assert d.boundary_weight == BW
    pw_ref, d2_ref = BR.boundary_weight(y.astype(np.uint8), valid, BW[2], BW[0], 1.0 / (2.0 * BW[1] ** 2))
    assert (d2_ref != BR.INF).any() and (d2_ref == BR.INF).any() and pw_ref.max() > 5
    # the rotation cut draws no contour: without the validity map it would
    assert not np.array_equal(pw_ref, BR.boundary_weight(y.astype(np.uint8), None, BW[2], BW[0], 1.0 / (2.0 * BW[1] ** 2))[0])
    params = {n: d.get_variable(n).astype(np.float64) for n in d.variable_names()}
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S, acc_mask=valid.reshape(B, -1))
    out = d.train_step(B, S, 0.01, apply_update=False, want_logits=True)
    torch.cuda.synchronize()
    M = B * S * S
    # the map the step made
    got_pw = d.pixel_weight[:M].cpu().numpy().reshape(B, S, S)
    assert _ulps(got_pw, pw_ref.astype(np.float32)).max() <= 1
    dec = []
    for i, L in enumerate(d.plan.layers):
        z = d.z[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        mr = d.mean_rstd[i].cpu().numpy().reshape(L.cout, 2)
        dc = {"pos": (z - mr[:, 0]) * mr[:, 1] > 0}
        if d._is_max(i):
            dc["idx"] = d.idx[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        dec.append(dc)

    def weighted(tn):
        """the loss written with torch ops and the reference's map, not the closed form"""
        for q in tn.params_list():
            q.grad = None
        logits = tn.forward(x.astype(np.float64), True)
        yy = torch.as_tensor(y.reshape(-1), dtype=torch.long)
        logp = torch.log_softmax(logits.reshape(-1, K), dim=1).gather(1, yy[:, None])[:, 0]
        l2 = sum(0.5 * (w_ ** 2).sum() for w_ in list(tn.w.values()) + list(tn.fcw.values()))
        pw = torch.as_tensor(pw_ref.reshape(-1), dtype=torch.float64)
        loss = (pw * torch.as_tensor(wc, dtype=torch.float64)[yy] * (1.0 - torch.exp(logp)) ** GAMMA * (-logp)).sum() / M + WD * l2
        plain = (torch.as_tensor(wc, dtype=torch.float64)[yy] * (1.0 - torch.exp(logp)) ** GAMMA * (-logp)).sum() / M + WD * l2
        loss.backward()
        return float(loss.detach()), logits.detach().numpy(), float(plain.detach())
    forced = _ForcedTorchNet(net, ch, K, params=params, dtype=torch.float64)
    forced.dec = dec
    loss_ref, logits_ref, loss_plain = weighted(forced)
    got_loss = d.loss_value(out["loss_parts"])
    print("boundary-weighted step %s: loss %.9g forced %.9g (without the map %.9g)" % (net, got_loss, loss_ref, loss_plain))
    assert abs(loss_ref - loss_plain) > 1e-2 * loss_plain
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
    # the unweighted quantities of the same step: the confusion matrix counts the valid pixels, each once
    cm = np.zeros((K, K), dtype=np.int64)
    ok = valid.reshape(-1) != 0
    np.add.at(cm, (y.reshape(-1)[ok], out["pred"].cpu().numpy().reshape(-1)[ok]), 1)
    np.testing.assert_array_equal(out["conf"].cpu().numpy().reshape(K, K), cm)
    # an eval forward ignores the option
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S)
    _, l1 = d.forward(B, S)
    l1 = l1.clone()
    d.set_boundary_weight(None)
    _, l0 = d.forward(B, S)
    assert torch.equal(l0, l1)


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES)
def test_step_engine_equals_op_level_and_repeats_bitwise(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    from drs_amd.engine import EngineNet
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    nets = [mk(), mk(engine=False), mk(), mk(), mk(engine=False)]
    assert isinstance(nets[0], EngineNet) and not isinstance(nets[1], EngineNet)
    for d in nets[:3]:                       # on top of class weights and the focal term ...
        d.set_class_weights(WEIGHTS[K])
        d.set_focal_gamma(2.0)
    for d in nets:                           # ... and alone
        d.set_boundary_weight(BW)
        assert d.boundary_weight == BW
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
                assert torch.equal(nets[ref].pixel_weight[:B * S * S], nets[i].pixel_weight[:B * S * S])
        assert not torch.equal(outs[3]["loss_parts"][:1], oo["loss_parts"][:1]) and not torch.equal(nets[3].grads, off.grads)
        assert not torch.equal(nets[0].grads, nets[3].grads)


def test_a_zero_or_never_set_leaves_a_training_trajectory_bitwise_unchanged():
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    a, b, c, e = mk(), mk(), mk(), mk(engine=False)
    b.set_boundary_weight((0, 2, 5))
    e.set_boundary_weight(0)
    c.set_boundary_weight(BW)
    assert type(a).__name__ == "EngineNet" and a.boundary_weight is None and b.boundary_weight is None and c.boundary_weight == BW
    mark = torch.full_like(a.pixel_weight, -7.0)
    for d in (a, b, e):
        d.pixel_weight.copy_(mark)
    for step in range(3):
        x, y, valid = _step_inputs(ch, K, B, S, 30 + step)
        xs, ys = x.reshape(B, -1), y.reshape(B, -1)
        oa, ob, oc, oe = _feed_step(a, xs, ys, S), _feed_step(b, xs, ys, S), _feed_step(c, xs, ys, S), _feed_step(e, xs, ys, S)
        torch.cuda.synchronize()
        for other, oo in ((b, ob), (e, oe)):
            for name in ("params", "mom", "grads", "bn"):
                assert torch.equal(getattr(a, name), getattr(other, name)), (name, step)
            assert torch.equal(oa["loss_parts"], oo["loss_parts"]) and torch.equal(oa["conf"], oo["conf"])
            assert torch.equal(other.pixel_weight, mark)          # off: no launch touches the buffer
        assert not torch.equal(a.grads, c.grads) and not torch.equal(oa["loss_parts"][:1], oc["loss_parts"][:1])


def test_bad_triples_are_rejected_by_both_nets():
    from drs_amd.net import DilatedNet
    nets = [DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV), DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV, engine=False)]
    for d in nets:
        for bad in (-2, 65, float("nan"), (1, 0), (1, 4, 17), (1, 4, 0), "2", (1, 2, 3, 4)):
            with pytest.raises(ValueError):
                d.set_boundary_weight(bad)
        assert d.boundary_weight is None
        d.set_boundary_weight((0.1, 2))
        assert d.boundary_weight == (0.1, 2.0, 6)
        d.set_boundary_weight(None)
        assert d.boundary_weight is None


# ------------------------------------------------------------------------------------------------- two ranks
DP = ("dilated8_grsl", 5, 6, 4, 21)
# The bounds of tests/test_gpu_dp.py::test_two_rank_step_equals_single_rank (loss 1e-6 ABSOLUTE, gradients 2e-3, parameters 1e-4) were
# set for ITS inputs and an unweighted loss: what separates a two-rank step from the single-rank one is a handful of ReLU signs / pool
# winners that flip on last-bit differences of the batch statistics -- a property of the forward pass, which the weight map
# does not touch -- and the size of what a flipped unit moves is the size of the gradient that flows through it.  So the case keeps
# that test's inputs (the same flips), adds the rotated-corner validity map, and takes a triple whose weights lie in [0.5, 1]: no
# gradient term is larger than in the unweighted step the bounds belong to.  Measured once while this test was written (relative
# gradient difference, same inputs): option off 1.4e-3, a = -0.5 1.2e-3, a = 0.25 1.8e-3, a = 1 2.6e-3; blob labels instead of random
# ones give 7.1e-3 with the option OFF and 8.0e-3 with a = 1, and a = 10 moves the loss to 18.1, where the same relative agreement of
# the loss (6e-8) is 1.1e-6 absolute: the differences are the parent's decision flips scaled by the weights, not the map's.
DP_BW = (-0.5, 3.0, 9)


def _dp_inputs():
    from test_gpu_dp import _inputs
    NET, CH, K, B, S = DP
    x, y = _inputs()
    return x, y, _rotated_corners(B, S).reshape(B, -1)


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import loops
    from drs_amd.dist import TorchComm, shard_slice
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    x, y, valid = _dp_inputs()
    sl = shard_slice(B, rank, world)
    d = DilatedNet(NET, CH, K, 0.005, b_max=B // world, s_max=S, device="cuda:0", seed=3, comm=comm)
    loops.setup_boundary_weight(d, DP_BW, comm, lambda *a: None)          # what the loops do: one agree on the triple's bits
    d.feed(x[sl], y[sl], S, acc_mask=valid[sl])
    res = d.train_step(B // world, S, 0.01)
    torch.cuda.synchronize()
    np.savez(out + "_rank%d.npz" % rank, grads=d.grads.cpu().numpy(), params=d.params.cpu().numpy(), bn=d.bn.cpu().numpy(),
             loss=d.loss_value(res["loss_parts"]), conf=res["conf"].cpu().numpy(), bw=np.asarray(d.boundary_weight))
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_step_follows_the_single_rank_step(tmp_path):
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(2, 30700 + os.getpid() % 1000, out), nprocs=2, join=True)
    x, y, valid = _dp_inputs()
    losses = {}
    for bw in (None, DP_BW):                # (the unweighted step too, to show below that the map mattered)
        d = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=3)
        d.set_boundary_weight(bw)
        d.feed(x, y, S, acc_mask=valid)
        res = d.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        losses[bw] = d.loss_value(res["loss_parts"])
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    assert tuple(r0["bw"]) == tuple(r1["bw"]) == DP_BW
    loss = losses[DP_BW]
    print("two ranks: loss %.9g (rank 0 %.9g), without the map %.9g" % (loss, float(r0["loss"]), losses[None]))
    assert abs(loss - losses[None]) > 1e-2 * losses[None]

    def rel(a, b):
        return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))
    # the bounds of tests/test_gpu_dp.py::test_two_rank_step_equals_single_rank
    assert abs(float(r0["loss"]) - loss) < 1e-6
    assert rel(r0["grads"], d.grads.cpu().numpy()) < 2e-3
    assert rel(r0["params"], d.params.cpu().numpy()) < 1e-4
    assert rel(r0["bn"], d.bn.cpu().numpy()) < 1e-6
    np.testing.assert_array_equal(r0["conf"], res["conf"].cpu().numpy())
    np.testing.assert_array_equal(r0["params"], r1["params"])


# ------------------------------------------------------------------------------------------------- loop
def test_train_loop_prints_the_weighted_loss_and_keeps_the_triple(tmp_path, capsys, monkeypatch):
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
        seen.append((self.logits[:M * K].cpu().numpy().astype(np.float64).reshape(M, K), self.labels[:M].cpu().numpy().reshape(B, S, S),
                     self.acc_mask[:M].cpu().numpy().reshape(B, S, S) if kw.get("use_acc_mask", True) else None,
                     out["loss_parts"].cpu().numpy().copy()))
        return out
    monkeypatch.setattr(EngineNet, "train_step", recording)
    out = str(tmp_path) + "/"
    net = loops.train(data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 4, WD, mean, std, "loss", "single_fixed",
                      [13], None, None, None, None, 20, out, 1, "dilated_grsl", "vaihingen", "none", device=DEV,
                      val_cache_dir=str(tmp_path), boundary_weight=(10, 2))
    text = capsys.readouterr().out
    assert "Boundary weight: a 10 sigma 2 R 6" in text and "Focal loss" not in text and "Class weights" not in text
    assert net.boundary_weight == (10.0, 2.0, 6) and net.focal_gamma == 0.0 and net.class_weights is None
    printed = [float(v) for v in re.findall(r"Training Minibatch: Loss= ([0-9.eE+-]+)", text)]
    assert len(printed) == len(seen) == 4
    for got, (lg, lab, valid, parts) in zip(printed, seen):
        pw, d2 = BR.boundary_weight(lab, valid, 6, 10.0, 1.0 / 8.0)
        assert (d2 != BR.INF).any()
        ce = focal_closed_form(lg, lab.reshape(-1).astype(np.int64), np.ones(K), 0.0)["ce"]
        want = float((pw.reshape(-1) * ce).sum() / ce.size) + WD * float(parts[1])
        plain = float(ce.mean()) + WD * float(parts[1])
        print("loop loss printed %.6f weighted %.6f cross-entropy %.6f" % (got, want, plain))
        assert abs(got - want) < 1e-4 * min(1.0, abs(want)) and abs(plain - want) > 1e-2 * plain
    assert os.path.isfile(out + "boundary_weight_step_4.npy") and not os.path.exists(out + "focal_gamma_step_4.npy")
    assert np.load(out + "boundary_weight_step_4.npy").tolist() == [10.0, 2.0, 6.0]
    # a resumed run trains the same loss and says so; a triple given on a resumed run replaces the restored one, and the log says that too
    args = (data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 5, WD, mean, std, "loss", "single_fixed", [13], None, None, None,
            None, 20, out, 1, "dilated_grsl", "vaihingen", out + "model-4")
    net2 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path))
    text = capsys.readouterr().out
    assert "Boundary weight (restored from " + out + "boundary_weight_step_4.npy): a 10 sigma 2 R 6" in text and net2.boundary_weight == (10.0, 2.0, 6)
    net3 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path), boundary_weight=(5, 4, 12), focal_gamma=2.0)
    text = capsys.readouterr().out
    assert "Boundary weight: a 5 sigma 4 R 12" in text and "replacing the triple restored from the checkpoint, a 10 sigma 2 R 6" in text
    assert "Focal loss: gamma 2" in text and net3.boundary_weight == (5.0, 4.0, 12) and net3.focal_gamma == 2.0
