"""-m gpu: the focal training loss from the kernels up: the three forms of the fused classifier against the fp64 closed
form (tests/focal_ref.py, itself held against fp64 autograd by tests/test_focal_loss_plan.py), steep logits, the bitwise no-op at
gamma = 0, a whole training step against fp64 autograd of the loss written with torch ops, engine = op level, two ranks, and the
training loop.

Definition held here: L = inv_n * sum over the pixels in the loss of wc[y] (1 - p_t)^gamma CE; gradient wrt the logits
wc[y] f (softmax - onehot) inv_n with f = m (1 + gamma p_t CE / q); inv_n stays 1 / the number of pixels the loss averages over.
Tolerances are the project's existing ones: single ops 1e-5 relative to the tensor's maximum and 1e-6 for the loss, whole nets 1e-4,
two ranks as tests/test_gpu_dp.py."""
import functools
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import torch_ref as TR

pytestmark = pytest.mark.gpu

from focal_ref import focal_closed_form   # noqa: E402
from gpu_util import DEV, dev, padded, rel_err, stream   # noqa: E402
from test_gpu_class_weights import PROBS, WEIGHTS, _case, _feed_step, _ForcedTorchNet   # noqa: E402  (helpers only: inputs, the decision-aligned graph)


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# the form table of tests/test_gpu_class_weights.py with the LDS-DMA form at B = 64, S = 64: M = 2^18 is the smallest pixel count that selects it
FORMS = {"valu-K2": (448, 2, 2, 13, 6), "valu-K3": (192, 3, 2, 15, 1), "mfma-K6": (256, 6, 3, 21, 0), "dma-K6-64x64x64": (256, 6, 64, 64, 0)}


def _check_form(form):
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    assert (form.startswith("dma")) == (K >= 4 and M >= (1 << 18) and C <= 256) and (form.startswith("valu")) == (K < 4)
    if form.startswith("dma"):
        assert M == 1 << 18


class _Run(object):
    """one launch of the classifier through `entry` and its slab reductions; every raw output kept"""

    RAW = ("logits", "pred", "gfeat", "dwp", "dbp", "lp", "conf")

    def __init__(self, lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, inv_n, wc, gamma, entry="drs_classifier_loss_focal"):
        M = B * S * S
        rows = lib.query("drs_classifier_rows", B, S)
        self.logits = torch.zeros(M * K, dtype=torch.float32, device=DEV)
        self.pred = torch.zeros(M, dtype=torch.uint8, device=DEV)
        self.gfeat = torch.zeros(M * C, dtype=torch.float32, device=DEV)
        self.dwp = torch.zeros(rows * C * K, dtype=torch.float32, device=DEV)
        self.dbp = torch.zeros(rows * K, dtype=torch.float32, device=DEV)
        self.lp = torch.zeros(rows, dtype=torch.float64, device=DEV)
        self.conf = torch.zeros(K * K, dtype=torch.int32, device=DEV)
        head = (fd.data_ptr(), B, S, P, C, 0, C, K, wdev.data_ptr(), bdev.data_ptr(), yd.data_ptr(), None if lmd is None else lmd.data_ptr(),
                amd.data_ptr(), inv_n)
        tail = (self.logits.data_ptr(), self.pred.data_ptr(), self.gfeat.data_ptr(), C, 0, self.dwp.data_ptr(), self.dbp.data_ptr(),
                self.lp.data_ptr(), self.conf.data_ptr(), stream())
        self.wc = None if wc is None else np.ascontiguousarray(wc, dtype=np.float32)
        wptr = None if wc is None else self.wc.ctypes.data
        mid = {"drs_classifier_loss": (), "drs_classifier_loss_weighted": (wptr,), "drs_classifier_loss_focal": (wptr, float(gamma))}[entry]
        lib.call(entry, *(head + mid + tail))
        self.dw = torch.zeros(C * K, dtype=torch.float32, device=DEV)
        self.db = torch.zeros(K, dtype=torch.float32, device=DEV)
        self.ls = torch.zeros(1, dtype=torch.float64, device=DEV)
        scr = torch.zeros(lib.query("drs_colsum_scratch_doubles", C * K), dtype=torch.float64, device=DEV)
        lib.call("drs_rows_reduce_f32", self.dwp.data_ptr(), rows, C * K, self.dw.data_ptr(), scr.data_ptr(), stream())
        lib.call("drs_rows_reduce_f32", self.dbp.data_ptr(), rows, K, self.db.data_ptr(), scr.data_ptr(), stream())
        lib.call("drs_sum_f64", self.lp.data_ptr(), rows, self.ls.data_ptr(), stream())
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=1)
def _moderate(form):
    """the inputs of a form, on the host in fp64 and on the device, and the plain launch: computed once, shared by the gammas, left unchanged"""
    from drs_amd import _lib
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    feat, w, bias, y, lm, am = _case(C, K, B, S, seed=C + K + S)
    n = float(lm.sum())
    d = dict(fd=padded(feat, P, fill=3.0) if P else dev(feat), yd=dev(y.reshape(-1)), amd=dev(am.reshape(-1)), lmd=dev(lm.reshape(-1)),
             wdev=dev(w), bdev=dev(bias), n=n)
    d["plain"] = _Run(_lib, d["fd"], B, S, P, C, K, d["wdev"], d["bdev"], d["yd"], d["lmd"], d["amd"], 1.0 / n, None, 0.0, entry="drs_classifier_loss")
    d["f64"] = feat.reshape(M, C).astype(np.float64)
    d["w64"] = w.astype(np.float64)
    d["lg_ref"] = d["f64"] @ d["w64"] + bias.astype(np.float64)
    d["yy"] = y.reshape(-1).astype(np.int64)
    d["inl"] = (d["yy"] < K) & (lm.reshape(-1) > 0)
    return d


def _reference(lg, yy, inl, wc, gamma, n, K):
    """loss and logit gradient [M][K] of the definition from logits `lg` (fp64); pixels outside the loss contribute nothing"""
    ref = focal_closed_form(lg, np.minimum(yy, K - 1), wc.astype(np.float64), gamma)
    return float((ref["term"] * inl).sum() / n), ref["grad"] * (inl / n)[:, None], ref


def _figures(r, d, loss_ref, gl, M, C, K):
    return dict(loss=abs(r.ls.item() / d["n"] - loss_ref) / abs(loss_ref), gfeat=rel_err(r.gfeat.cpu().numpy().reshape(M, C), gl @ d["w64"].T),
                dw=rel_err(r.dw.cpu().numpy().reshape(C, K), d["f64"].T @ gl), db=rel_err(r.db.cpu().numpy(), gl.sum(axis=0)))


MODERATE = [(f, g) for f in FORMS for g in ((0.5, 1.0, 2.0, 5.0) if f == "mfma-K6" else (0.5, 2.0))]


@pytest.mark.parametrize("form,gamma", MODERATE, ids=["%s-g%g" % fg for fg in MODERATE])
def test_focal_classifier_against_fp64_numpy(lib, form, gamma):
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    d = _moderate(form)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32)
    r = _Run(lib, d["fd"], B, S, P, C, K, d["wdev"], d["bdev"], d["yd"], d["lmd"], d["amd"], 1.0 / d["n"], wc, gamma)
    plain = d["plain"]
    # not modulated: logits, arg-max, confusion matrix -- bit for bit those of drs_classifier_loss
    assert torch.equal(r.logits, plain.logits) and torch.equal(r.pred, plain.pred) and torch.equal(r.conf, plain.conf)
    assert rel_err(r.logits.cpu().numpy().reshape(M, K), d["lg_ref"]) < 1e-5
    yy, inl = d["yy"], d["inl"]
    loss_ref, gl, ref = _reference(d["lg_ref"], yy, inl, wc, gamma, d["n"], K)
    figures = _figures(r, d, loss_ref, gl, M, C, K)
    print("focal classifier %s gamma=%g: %s" % (form, gamma, figures))
    zero = int(np.flatnonzero(wc == 0)[0])
    assert not r.gfeat.view(M, C)[torch.from_numpy(~inl | (yy == zero)).to(DEV)].any()      # weight 0 / not in the loss: exact zeros
    assert (wc == 0).sum() == 1 and (inl & (yy == zero)).sum() > 10 and not (yy < K).all() and not inl.all()
    assert not (gl[inl & (yy == zero)] != 0).any() and (gl[inl & (yy != zero)] != 0).all()
    weighted_ce = float((wc.astype(np.float64)[np.minimum(yy, K - 1)] * ref["ce"] * inl).sum() / d["n"])
    assert abs(loss_ref - weighted_ce) > 1e-2 * weighted_ce          # focal changes the loss by more than 1 %
    assert np.isfinite(r.gfeat.cpu().numpy()).all()
    assert figures["loss"] < 1e-6
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5


# ------------------------------------------------------------------------------------------------- steep logits
STEEP_SCALE = 16.0        # classifier weights x 16: logits of standard deviation ~ 16 (chosen on the CPU: 61 / 87 pixels of the two regimes at K = 2, 41 / 630 at K = 6)


@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("form", ["valu-K2", "mfma-K6"])
def test_steep_logits_teacher_forced(lib, form, gamma):
    """fp32 rounding of logits this large is not this feature's subject: the fp64 formula is evaluated on the DEVICE'S OWN logits"""
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    M = B * S * S
    feat, w, bias, y, lm, am = _case(C, K, B, S, seed=3 * C + K)
    w = (w * STEEP_SCALE).astype(np.float32)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32)
    n = float(lm.sum())
    yy = y.reshape(-1).astype(np.int64)
    inl = (yy < K) & (lm.reshape(-1) > 0)
    d = dict(n=n, f64=feat.reshape(M, C).astype(np.float64), w64=w.astype(np.float64))
    # the reference alone shows the two regimes
    ref0 = focal_closed_form(d["f64"] @ d["w64"] + bias.astype(np.float64), np.minimum(yy, K - 1), wc.astype(np.float64), gamma)
    n_conf, n_wrong = int((inl & (ref0["q"] < 1e-6)).sum()), int((inl & (ref0["pt"] < 1e-4)).sum())
    print("steep %s: in-loss pixels with q < 1e-6: %d, with p_t < 1e-4: %d" % (form, n_conf, n_wrong))
    assert n_conf > 10 and n_wrong > 10
    fd = padded(feat, P, fill=3.0) if P else dev(feat)
    r = _Run(lib, fd, B, S, P, C, K, dev(w), dev(bias), dev(y.reshape(-1)), dev(lm.reshape(-1)), dev(am.reshape(-1)), 1.0 / n, wc, gamma)
    for name in ("logits", "gfeat", "dwp", "dbp", "lp", "dw", "db", "ls"):
        assert bool(torch.isfinite(getattr(r, name)).all()), name
    lg = r.logits.cpu().numpy().astype(np.float64).reshape(M, K)
    loss_ref, gl, ref = _reference(lg, yy, inl, wc, gamma, n, K)
    assert int((inl & (ref["q"] < 1e-6)).sum()) > 10 and int((inl & (ref["pt"] < 1e-4)).sum()) > 10
    figures = _figures(r, d, loss_ref, gl, M, C, K)
    print("steep focal classifier %s gamma=%g: %s" % (form, gamma, figures))
    assert figures["loss"] < 1e-6
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5


# ------------------------------------------------------------------------------------------------- gamma = 0
@pytest.mark.parametrize("form", list(FORMS))
def test_gamma_zero_is_bitwise_the_weighted_and_the_unweighted_call(lib, form):
    _check_form(form)
    C, K, B, S, P = FORMS[form]
    feat, w, bias, y, lm, am = _case(C, K, B, S, seed=7 + K)
    fd = padded(feat, P, fill=3.0) if P else dev(feat)
    yd, amd, lmd, wdev, bdev = dev(y.reshape(-1)), dev(am.reshape(-1)), dev(lm.reshape(-1)), dev(w), dev(bias)
    inv_n = 1.0 / float(lm.sum())
    args = (lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, inv_n)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32)
    plain = _Run(*args, None, 0.0, entry="drs_classifier_loss")
    weighted = _Run(*args, wc, 0.0, entry="drs_classifier_loss_weighted")
    assert float(plain.gfeat.abs().max()) > 0 and float(plain.ls.item()) > 0 and not torch.equal(plain.gfeat, weighted.gfeat)
    for base, w_ in ((plain, None), (weighted, wc)):
        r = _Run(*args, w_, 0.0)
        for name in _Run.RAW + ("dw", "db", "ls"):
            assert torch.equal(getattr(r, name), getattr(base, name)), (name, w_)
    # and gamma = 2 changes the gradients, not the logits' bits
    for base, w_ in ((plain, None), (weighted, wc)):
        r = _Run(*args, w_, 2.0)
        assert not torch.equal(r.gfeat, base.gfeat) and not torch.equal(r.ls, base.ls) and torch.equal(r.logits, base.logits)
        assert torch.equal(r.pred, base.pred) and torch.equal(r.conf, base.conf)


def test_gamma_zero_leaves_a_training_trajectory_bitwise_unchanged():
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    a = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7)
    b = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7)
    c = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7)
    b.set_focal_gamma(0)
    c.set_focal_gamma(2)
    assert type(a).__name__ == "EngineNet" and a.focal_gamma == 0.0 and b.focal_gamma == 0.0 and c.focal_gamma == 2.0
    rng = np.random.default_rng(2)
    for step in range(3):
        x = rng.normal(size=(B, S * S * ch)).astype(np.float32)
        y = rng.integers(0, K, size=(B, S * S))
        oa, ob, oc = _feed_step(a, x, y, S), _feed_step(b, x, y, S), _feed_step(c, x, y, S)
        torch.cuda.synchronize()
        for name in ("params", "mom", "grads", "bn"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (name, step)
        assert torch.equal(oa["loss_parts"], ob["loss_parts"]) and torch.equal(oa["conf"], ob["conf"])
        assert not torch.equal(a.grads, c.grads) and not torch.equal(oa["loss_parts"][:1], oc["loss_parts"][:1])


def test_bad_gamma_is_rejected(lib):
    C, K, B, S, P = FORMS["mfma-K6"]
    feat, w, bias, y, lm, am = _case(C, K, 1, 8, seed=1)
    fd, yd, amd, wdev, bdev = dev(feat), dev(y.reshape(-1)), dev(am.reshape(-1)), dev(w), dev(bias)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), 8.5):
        with pytest.raises(lib.DrsError, match="DRS_ERR_ARG"):
            _Run(lib, fd, 1, 8, 0, C, K, wdev, bdev, yd, None, amd, 1.0 / 64, None, bad)
    _Run(lib, fd, 1, 8, 0, C, K, wdev, bdev, yd, None, amd, 1.0 / 64, None, 8.0)
    from drs_amd.net import DilatedNet
    nets = [DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV), DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV, engine=False)]
    for d in nets:
        for bad in (-1, float("nan"), float("inf"), 9, "2"):
            with pytest.raises(ValueError):
                d.set_focal_gamma(bad)
        assert d.focal_gamma == 0.0
        d.set_focal_gamma(0.1)
        assert d.focal_gamma == float(np.float32(0.1))
        d.set_focal_gamma(None)
        assert d.focal_gamma == 0.0
    for bad in (-1.0, float("nan"), float("inf"), 8.5):
        assert lib.query("drs_net_set_focal_gamma", nets[0].h, bad) == 1
    assert nets[0].focal_gamma == 0.0


# ------------------------------------------------------------------------------------------------- the step
def _balanced(y, K):
    from drs_amd import patches as P
    return P.check_class_weights(list(P.class_weights(np.bincount(y.reshape(-1), minlength=K), "balanced")), K)


@pytest.mark.parametrize("net,ch,K,B,S", [("dilated_grsl", 5, 6, 3, 19), ("dilated_icpr_rate6_densely", 4, 2, 2, 21)],
                         ids=["Dilated6Pooling", "DenseDilated6"])
def test_focal_training_step_against_fp64_autograd(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    WD, GAMMA = 0.005, 2.0
    rng = np.random.default_rng(11)
    d = DilatedNet(net, ch, K, WD, b_max=B, s_max=S, device=DEV, seed=11)
    x = rng.normal(size=(B, S, S, ch)).astype(np.float32)
    p = np.asarray([0.6, 0.4] if K == 2 else [0.45, 0.25, 0.15, 0.08, 0.05, 0.02])
    y = rng.choice(K, size=(B, S, S), p=p)
    wc = _balanced(y, K)
    assert wc.max() > 1.2 * wc.min()
    d.set_class_weights(wc)
    d.set_focal_gamma(GAMMA)
    params = {n: d.get_variable(n).astype(np.float64) for n in d.variable_names()}
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S)
    out = d.train_step(B, S, 0.01, apply_update=False, want_logits=True)
    torch.cuda.synchronize()
    M = B * S * S
    dec = []
    for i, L in enumerate(d.plan.layers):
        z = d.z[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        mr = d.mean_rstd[i].cpu().numpy().reshape(L.cout, 2)
        dc = {"pos": (z - mr[:, 0]) * mr[:, 1] > 0}
        if d._is_max(i):
            dc["idx"] = d.idx[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        dec.append(dc)

    def focal(tn):
        """the loss written with torch ops, not the closed form"""
        for q in tn.params_list():
            q.grad = None
        logits = tn.forward(x.astype(np.float64), True)
        yy = torch.as_tensor(y.reshape(-1), dtype=torch.long)
        logp = torch.log_softmax(logits.reshape(-1, K), dim=1).gather(1, yy[:, None])[:, 0]
        l2 = sum(0.5 * (w_ ** 2).sum() for w_ in list(tn.w.values()) + list(tn.fcw.values()))
        loss = (torch.as_tensor(wc, dtype=torch.float64)[yy] * (1.0 - torch.exp(logp)) ** GAMMA * (-logp)).sum() / M + WD * l2
        loss.backward()
        return float(loss.detach()), logits.detach().numpy()
    free = TR.TorchNet(net, ch, K, params=params, dtype=torch.float64)
    loss_free, logits_free = focal(free)
    got_loss = d.loss_value(out["loss_parts"])
    lg = d.logits[:M * K].cpu().numpy().reshape(B, S, S, K)
    assert rel_err(lg, logits_free) < 1e-3
    assert abs(got_loss - loss_free) < 1e-4 * abs(loss_free)
    forced = _ForcedTorchNet(net, ch, K, params=params, dtype=torch.float64)
    forced.dec = dec
    loss_ref, logits_ref = focal(forced)
    print("focal step %s: loss %.9g free %.9g forced %.9g" % (net, got_loss, loss_free, loss_ref))
    assert abs(got_loss - loss_ref) < 1e-4 * abs(loss_ref)
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
    # the unmodulated quantities of the same step
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (y.reshape(-1), out["pred"].cpu().numpy().reshape(-1)), 1)
    np.testing.assert_array_equal(out["conf"].cpu().numpy(), cm)
    # an eval forward ignores gamma
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S)
    _, l1 = d.forward(B, S)
    l1 = l1.clone()
    d.set_focal_gamma(0)
    _, l0 = d.forward(B, S)
    assert torch.equal(l0, l1)


@pytest.mark.parametrize("net,ch,K,B,S", [("dilated_grsl", 5, 6, 3, 19), ("dilated_icpr_rate6_densely", 4, 2, 2, 21)])
def test_focal_step_engine_equals_op_level_and_repeats_bitwise(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    from drs_amd.engine import EngineNet
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    nets = [mk(), mk(engine=False), mk(), mk(), mk(engine=False)]
    assert isinstance(nets[0], EngineNet) and not isinstance(nets[1], EngineNet)
    for d in nets[:3]:                       # with class weights ...
        d.set_class_weights(WEIGHTS[K])
    for d in nets:                           # ... and without
        d.set_focal_gamma(2.0)
        assert d.focal_gamma == 2.0
    weighted = mk()
    weighted.set_class_weights(WEIGHTS[K])
    rng = np.random.default_rng(1)
    for step in range(2):
        x = rng.normal(size=(B, S * S * ch)).astype(np.float32)
        y = rng.integers(0, K, size=(B, S * S))
        outs = [_feed_step(d, x, y, S, want_logits=True) for d in nets]
        ow = _feed_step(weighted, x, y, S)
        torch.cuda.synchronize()
        for ref, others in ((0, (1, 2)), (3, (4,))):
            for i in others:
                for name in ("params", "grads", "mom", "bn"):
                    assert torch.equal(getattr(nets[ref], name), getattr(nets[i], name)), (name, step, i)
                assert torch.equal(outs[ref]["loss_parts"], outs[i]["loss_parts"]) and torch.equal(outs[ref]["conf"], outs[i]["conf"])
                assert torch.equal(nets[ref].logits[:B * S * S * K], nets[i].logits[:B * S * S * K])
        assert not torch.equal(outs[0]["loss_parts"][:1], ow["loss_parts"][:1]) and not torch.equal(nets[0].grads, weighted.grads)
        assert not torch.equal(nets[0].grads, nets[3].grads)


# ------------------------------------------------------------------------------------------------- two ranks
DP = ("dilated8_grsl", 5, 6, 4, 21)
DP_GAMMA = 2.0


def _dp_inputs():
    rng = np.random.default_rng(0)
    NET, CH, K, B, S = DP
    y = rng.choice(K, size=(B, S * S), p=[0.5, 0.25, 0.12, 0.08, 0.04, 0.01])
    return rng.normal(size=(B, S * S * CH)).astype(np.float32), y


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd import patches as P
    from drs_amd.dist import TorchComm, shard_slice
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    x, y = _dp_inputs()
    wc = _balanced(y, K)
    g = P.check_focal_gamma(DP_GAMMA)
    comm.agree([int(np.asarray(g, dtype=np.float32).view(np.uint32))], "focal gamma")        # what the loops do: one agree on gamma's bits
    sl = shard_slice(B, rank, world)
    d = DilatedNet(NET, CH, K, 0.005, b_max=B // world, s_max=S, device="cuda:0", seed=3, comm=comm)
    d.set_class_weights(wc)
    d.set_focal_gamma(g)
    d.feed(x[sl], y[sl], S)
    res = d.train_step(B // world, S, 0.01)
    torch.cuda.synchronize()
    np.savez(out + "_rank%d.npz" % rank, grads=d.grads.cpu().numpy(), params=d.params.cpu().numpy(), bn=d.bn.cpu().numpy(),
             loss=d.loss_value(res["loss_parts"]), conf=res["conf"].cpu().numpy(), gamma=d.focal_gamma)
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_focal_step_follows_the_single_rank_step(tmp_path):
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(2, 29600 + os.getpid() % 1000, out), nprocs=2, join=True)
    x, y = _dp_inputs()
    losses = {}
    for g in (0.0, DP_GAMMA):               # (the unmodulated step too, to show below that gamma mattered)
        d = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=3)
        d.set_class_weights(_balanced(y, K))
        d.set_focal_gamma(g)
        d.feed(x, y, S)
        res = d.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        losses[g] = d.loss_value(res["loss_parts"])
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    assert float(r0["gamma"]) == float(r1["gamma"]) == DP_GAMMA
    loss = losses[DP_GAMMA]
    assert abs(loss - losses[0.0]) > 1e-2 * losses[0.0]

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
def test_train_loop_prints_the_focal_loss_and_keeps_gamma(tmp_path, capsys, monkeypatch):
    from drs_amd import loops, sampling as SP
    from drs_amd.engine import EngineNet
    from drs_amd.synthetic import make_tile
    K, WD, GAMMA = 6, 0.005, 2.0
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
        seen.append((self.logits[:M * K].cpu().numpy().astype(np.float64).reshape(M, K), self.labels[:M].cpu().numpy().astype(np.int64),
                     out["loss_parts"].cpu().numpy().copy()))
        return out
    monkeypatch.setattr(EngineNet, "train_step", recording)
    out = str(tmp_path) + "/"
    net = loops.train(data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 4, WD, mean, std, "loss", "single_fixed",
                      [13], None, None, None, None, 20, out, 1, "dilated_grsl", "vaihingen", "none", device=DEV,
                      val_cache_dir=str(tmp_path), focal_gamma=GAMMA)
    text = capsys.readouterr().out
    assert "Focal loss: gamma 2" in text and "Class weights" not in text
    assert net.focal_gamma == GAMMA and net.class_weights is None
    printed = [float(v) for v in re.findall(r"Training Minibatch: Loss= ([0-9.eE+-]+)", text)]
    assert len(printed) == len(seen) == 4
    for got, (lg, yy, parts) in zip(printed, seen):
        ref = focal_closed_form(lg, yy, np.ones(K), GAMMA)
        want = float(ref["term"].sum() / len(yy)) + WD * float(parts[1])
        plain = float(ref["ce"].mean()) + WD * float(parts[1])
        print("loop loss printed %.6f focal %.6f cross-entropy %.6f" % (got, want, plain))
        assert abs(got - want) < 1e-4 * min(1.0, abs(want)) and abs(plain - want) > 1e-2 * plain
    assert os.path.isfile(out + "focal_gamma_step_4.npy") and not os.path.exists(out + "class_weights_step_4.npy")
    assert float(np.load(out + "focal_gamma_step_4.npy")) == GAMMA
    # a resumed run trains the same loss and says so; a gamma given on a resumed run replaces the restored one, and the log says that too
    args = (data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 5, WD, mean, std, "loss", "single_fixed", [13], None, None, None,
            None, 20, out, 1, "dilated_grsl", "vaihingen", out + "model-4")
    net2 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path))
    text = capsys.readouterr().out
    assert "Focal loss (restored from " + out + "focal_gamma_step_4.npy): gamma 2" in text and net2.focal_gamma == GAMMA
    net3 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path), focal_gamma=0.5, class_weights="balanced")
    text = capsys.readouterr().out
    assert "Focal loss: gamma 0.5" in text and "replacing the gamma restored from the checkpoint, 2" in text and "Class weights (balanced)" in text
    assert net3.focal_gamma == 0.5 and net3.class_weights is not None
