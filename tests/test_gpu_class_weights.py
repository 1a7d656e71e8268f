"""-m gpu: the class-weighted training loss from the kernels up: the three forms of the fused classifier against fp64
numpy, the bitwise no-op without weights, a whole training step against fp64 autograd of the weighted loss, engine = op level, the
label histogram, two ranks, and the training loop.

Definition held here: L = inv_n * sum over the pixels in the loss of wc[y] * CE, gradient wrt the logits wc[y] (softmax - onehot) inv_n;
inv_n stays 1 / the number of pixels the loss averages over.  Tolerances are the project's existing ones: single ops 1e-5 relative to
the tensor's maximum and 1e-6 for the loss (tests/test_gpu_ops.py, tests/test_gpu_headline_step.py), whole nets 1e-4
(tests/test_gpu_net.py), two ranks as tests/test_gpu_dp.py."""
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from oracle import nets as onets
from oracle import torch_ref as TR
from oracle.tf_ops import BN_DECAY, BN_EPS

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, padded, rel_err, stream   # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# the shape selects the form (csrc/pointwise.hip drs_classifier_loss_weighted): K < 4 the vector-ALU form, K >= 4 the matrix-core form,
# K >= 4 from 2^18 pixels (C <= 256) the LDS-DMA form
# (K = 2 is the exact-class-count instantiation of the vector-ALU form, K = 3 its eight-slot one)
FORMS = {"valu-K2": (448, 2, 2, 13, 6), "valu-K3": (192, 3, 2, 15, 1), "mfma-K6": (256, 6, 3, 21, 0), "dma-K6-128x64x64": (256, 6, 128, 64, 0)}
WEIGHTS = {2: [0.0, 3.5], 3: [2.0, 0.0, 0.5], 6: [0.5, 2.0, 0.0, 1.25, 7.0, 1.0]}          # every vector has ONE weight equal to 0
PROBS = {2: [0.55, 0.45], 3: [0.6, 0.3, 0.1], 6: [0.5, 0.25, 0.12, 0.08, 0.04, 0.01]}           # imbalanced, one rare class


def _case(C, K, B, S, seed):
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal(size=(B, S, S, C), dtype=np.float32)
    w = (rng.normal(size=(C, K)) / np.sqrt(C)).astype(np.float32)
    bias = (rng.normal(size=K) * 0.1).astype(np.float32)
    y = rng.choice(K, size=(B, S, S), p=np.asarray(PROBS[K])).astype(np.uint8)
    out = rng.random(size=y.shape) < 0.03                      # labels outside [0, K): never in the loss, never in the confusion matrix
    y[out] = rng.choice([K, 255], size=int(out.sum())).astype(np.uint8)
    lm = (rng.random(size=y.shape) < 0.7).astype(np.uint8)
    am = (rng.random(size=y.shape) < 0.8).astype(np.uint8)
    return feat, w, bias, y, lm, am


class _Run(object):
    """one launch of the classifier and its slab reductions; every raw output kept"""

    def __init__(self, lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, inv_n, wc, entry="drs_classifier_loss_weighted"):
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
        if entry == "drs_classifier_loss":
            lib.call(entry, *(head + tail))
        else:
            self.wc = None if wc is None else np.ascontiguousarray(wc, dtype=np.float32)
            lib.call(entry, *(head + (None if wc is None else self.wc.ctypes.data,) + tail))
        self.dw = torch.zeros(C * K, dtype=torch.float32, device=DEV)
        self.db = torch.zeros(K, dtype=torch.float32, device=DEV)
        self.ls = torch.zeros(1, dtype=torch.float64, device=DEV)
        scr = torch.zeros(lib.query("drs_colsum_scratch_doubles", C * K), dtype=torch.float64, device=DEV)
        lib.call("drs_rows_reduce_f32", self.dwp.data_ptr(), rows, C * K, self.dw.data_ptr(), scr.data_ptr(), stream())
        lib.call("drs_rows_reduce_f32", self.dbp.data_ptr(), rows, K, self.db.data_ptr(), scr.data_ptr(), stream())
        lib.call("drs_sum_f64", self.lp.data_ptr(), rows, self.ls.data_ptr(), stream())
        torch.cuda.synchronize()

    RAW = ("logits", "pred", "gfeat", "dwp", "dbp", "lp", "conf")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "lossmask"])
@pytest.mark.parametrize("form", list(FORMS))
def test_weighted_classifier_against_fp64_numpy(lib, form, masked):
    C, K, B, S, P = FORMS[form]
    feat, w, bias, y, lm, am = _case(C, K, B, S, seed=C + K + S)
    M = B * S * S
    assert (form.startswith("dma")) == (K >= 4 and M >= (1 << 18) and C <= 256) and (form.startswith("valu")) == (K < 4)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32)
    n = float(lm.sum()) if masked else float(M)
    fd = padded(feat, P, fill=3.0) if P else dev(feat)
    yd, amd, wdev, bdev = dev(y.reshape(-1)), dev(am.reshape(-1)), dev(w), dev(bias)
    lmd = dev(lm.reshape(-1)) if masked else None
    r = _Run(lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, 1.0 / n, wc)
    plain = _Run(lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, 1.0 / n, None, entry="drs_classifier_loss")
    # not weighted: logits, arg-max, confusion matrix -- bit for bit those of the unweighted call, and right
    assert torch.equal(r.logits, plain.logits) and torch.equal(r.pred, plain.pred) and torch.equal(r.conf, plain.conf)
    f64 = feat.reshape(M, C).astype(np.float64)
    w64 = w.astype(np.float64)
    lg_ref = f64 @ w64 + bias.astype(np.float64)
    lg = r.logits.cpu().numpy().reshape(M, K)
    assert rel_err(lg, lg_ref) < 1e-5
    ph = r.pred.cpu().numpy()
    np.testing.assert_array_equal(ph, lg.argmax(axis=1))
    yy, ok = y.reshape(-1).astype(np.int64), y.reshape(-1) < K
    cm = np.zeros((K, K), dtype=np.int64)
    sel = ok & (am.reshape(-1) > 0)
    np.add.at(cm, (yy[sel], ph[sel]), 1)
    np.testing.assert_array_equal(r.conf.cpu().numpy().reshape(K, K), cm)
    # weighted: loss and every gradient, fp64
    inl = ok & ((lm.reshape(-1) > 0) if masked else True)
    yc = np.minimum(yy, K - 1)
    mx = lg_ref.max(axis=1, keepdims=True)
    e = np.exp(lg_ref - mx)
    se = e.sum(axis=1, keepdims=True)
    ce = (np.log(se) + mx)[:, 0] - lg_ref[np.arange(M), yc]
    wy = wc.astype(np.float64)[yc] * inl
    loss_ref = float((wy * ce).sum() / n)
    onehot = np.zeros((M, K))
    onehot[np.arange(M), yc] = 1.0
    gl = (e / se - onehot) * (wy / n)[:, None]
    loss = r.ls.item() / n
    figures = dict(loss=abs(loss - loss_ref) / abs(loss_ref), gfeat=rel_err(r.gfeat.cpu().numpy().reshape(M, C), gl @ w64.T),
                   dw=rel_err(r.dw.cpu().numpy().reshape(C, K), f64.T @ gl), db=rel_err(r.db.cpu().numpy(), gl.sum(axis=0)))
    print("weighted classifier %s masked=%s: %s" % (form, masked, figures))
    assert not r.gfeat.view(M, C)[torch.from_numpy(~inl | (yy == int(np.flatnonzero(wc == 0)[0]))).to(DEV)].any()      # weight 0 / not in the loss: exact zeros
    # the case has one weight equal to 0 with pixels of that class in the loss, a weight above 1 likewise, and labels outside [0, K)
    zero = int(np.flatnonzero(wc == 0)[0])
    assert (wc == 0).sum() == 1 and (inl & (yy == zero)).sum() > 10 and (inl & (wc[yc] > 1)).sum() > 10 and not ok.all()
    assert not (gl[inl & (yy == zero)] != 0).any() and (gl[inl & (yy != zero)] != 0).all()
    assert abs(loss_ref - float((inl * ce).sum() / n)) > 1e-2 * loss_ref          # (and the weights do change the loss)
    assert figures["loss"] < 1e-6
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5


@pytest.mark.parametrize("form", list(FORMS))
def test_null_and_all_ones_weights_are_bitwise_the_unweighted_call(lib, form):
    C, K, B, S, P = FORMS[form]
    feat, w, bias, y, lm, am = _case(C, K, B, S, seed=7 + K)
    fd = padded(feat, P, fill=3.0) if P else dev(feat)
    yd, amd, lmd, wdev, bdev = dev(y.reshape(-1)), dev(am.reshape(-1)), dev(lm.reshape(-1)), dev(w), dev(bias)
    inv_n = 1.0 / float(lm.sum())
    base = _Run(lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, inv_n, None, entry="drs_classifier_loss")
    assert float(base.gfeat.abs().max()) > 0 and float(base.ls.item()) > 0
    for wc in (None, np.ones(K, dtype=np.float32)):
        r = _Run(lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, inv_n, wc)
        for name in _Run.RAW + ("dw", "db", "ls"):
            assert torch.equal(getattr(r, name), getattr(base, name)), (name, wc)
    # and a weight that is not one changes the gradients
    other = np.ones(K, dtype=np.float32)
    other[0] = 2.0
    r = _Run(lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, inv_n, other)
    assert not torch.equal(r.gfeat, base.gfeat) and torch.equal(r.logits, base.logits)


def test_bad_weights_are_rejected(lib):
    C, K, B, S, P = FORMS["mfma-K6"]
    feat, w, bias, y, lm, am = _case(C, K, 1, 8, seed=1)
    fd, yd, amd, wdev, bdev = dev(feat), dev(y.reshape(-1)), dev(am.reshape(-1)), dev(w), dev(bias)
    for bad in ([1, 1, -0.5, 1, 1, 1], [1, float("nan"), 1, 1, 1, 1], [1, 1, 1, float("inf"), 1, 1]):
        with pytest.raises(lib.DrsError, match="DRS_ERR_ARG"):
            _Run(lib, fd, 1, 8, 0, C, K, wdev, bdev, yd, None, amd, 1.0 / 64, np.asarray(bad, dtype=np.float32))
    from drs_amd.net import DilatedNet
    d = DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV)
    with pytest.raises(ValueError):
        d.set_class_weights([1.0, 2.0])
    with pytest.raises(ValueError):
        d.set_class_weights([1.0] * 5 + [-1.0])
    import ctypes as C_
    w5 = (C_.c_float * 5)(1, 1, 1, 1, 1)
    assert lib.query("drs_net_set_class_weights", d.h, C_.cast(w5, C_.c_void_p), 5) == 1            # K must be the net's
    assert d.class_weights is None
    d.set_class_weights([1, 2, 3, 4, 5, 6])
    np.testing.assert_array_equal(d.class_weights, np.asarray([1, 2, 3, 4, 5, 6], dtype=np.float32))
    d.set_class_weights(None)
    assert d.class_weights is None


# ------------------------------------------------------------------------------------------------- the step
def _feed_step(d, x, y, S, **kw):
    d.feed(x, y, S)
    return d.train_step(x.shape[0], S, 0.01, **kw)


def test_all_ones_weights_leave_a_training_trajectory_bitwise_unchanged():
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    a = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7)
    b = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7)
    b.set_class_weights(np.ones(K))
    assert type(a).__name__ == "EngineNet" and a.class_weights is None and b.class_weights is not None
    rng = np.random.default_rng(2)
    for step in range(3):
        x = rng.normal(size=(B, S * S * ch)).astype(np.float32)
        y = rng.integers(0, K, size=(B, S * S))
        oa, ob = _feed_step(a, x, y, S), _feed_step(b, x, y, S)
        torch.cuda.synchronize()
        for name in ("params", "mom", "grads", "bn"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (name, step)
        assert torch.equal(oa["loss_parts"], ob["loss_parts"]) and torch.equal(oa["conf"], ob["conf"])


@pytest.mark.parametrize("net,ch,K,B,S", [("dilated_grsl", 5, 6, 3, 19), ("dilated_icpr_rate6_densely", 4, 2, 2, 21)])
def test_weighted_step_engine_equals_op_level_and_repeats_bitwise(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    from drs_amd.engine import EngineNet
    nets = [DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7), DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, engine=False),
            DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7)]
    assert isinstance(nets[0], EngineNet) and not isinstance(nets[1], EngineNet)
    for d in nets:
        d.set_class_weights(WEIGHTS[K])
        np.testing.assert_array_equal(d.class_weights, np.asarray(WEIGHTS[K], dtype=np.float32))
    plain = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7)
    rng = np.random.default_rng(1)
    for step in range(2):
        x = rng.normal(size=(B, S * S * ch)).astype(np.float32)
        y = rng.integers(0, K, size=(B, S * S))
        outs = [_feed_step(d, x, y, S, want_logits=True) for d in nets]
        op = _feed_step(plain, x, y, S)
        torch.cuda.synchronize()
        for other, o2 in zip(nets[1:], outs[1:]):
            for name in ("params", "grads", "mom", "bn"):
                assert torch.equal(getattr(nets[0], name), getattr(other, name)), (name, step)
            assert torch.equal(outs[0]["loss_parts"], o2["loss_parts"]) and torch.equal(outs[0]["conf"], o2["conf"])
            assert torch.equal(nets[0].logits[:B * S * S * K], other.logits[:B * S * S * K])
        assert not torch.equal(outs[0]["loss_parts"][:1], op["loss_parts"][:1]) and not torch.equal(nets[0].grads, plain.grads)


class _ForcedTorchNet(TR.TorchNet):
    """oracle/torch_ref.py's graph with the device's discrete decisions (activation signs, pool winners) imposed, so that autograd's
    gradients compare tightly (the decision-aligned method of tests/test_gpu_net.py): only the block differs, `forward` is the oracle's"""
    dec = None

    def _block(self, li, inp, is_training):
        name, k, ci, co, r = self.convs[li]
        pb, pa = onets.same_pad(k, r)
        z = F.conv2d(F.pad(inp, (pb, pa, pb, pa)), self.w[name], self.b[name], dilation=r)
        y = F.batch_norm(z, self.mm[name], self.mv[name], None, None, training=is_training, momentum=1.0 - BN_DECAY, eps=BN_EPS)
        pos = torch.from_numpy(self.dec[li]["pos"]).permute(0, 3, 1, 2)
        y = torch.where(pos, y, (0.0 if self.spec["act"] == "relu" else 0.1) * y)
        if self.spec["pool"]:
            idx = torch.from_numpy(self.dec[li]["idx"].astype(np.int64)).permute(0, 3, 1, 2)
            H, W = y.shape[2:]
            yp = F.pad(y, (1, 1, 1, 1))
            stack = torch.stack([yp[:, :, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], dim=0)
            y = torch.gather(stack, 0, idx[None])[0]
        return y


@pytest.mark.parametrize("net,ch,K,B,S", [("dilated_grsl", 5, 6, 3, 19), ("dilated_icpr_rate6_densely", 4, 2, 2, 21)],
                         ids=["Dilated6Pooling", "DenseDilated6"])
def test_weighted_training_step_against_fp64_autograd(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    WD = 0.005
    rng = np.random.default_rng(11)
    d = DilatedNet(net, ch, K, WD, b_max=B, s_max=S, device=DEV, seed=11)
    x = rng.normal(size=(B, S, S, ch)).astype(np.float32)
    p = np.asarray([0.6, 0.4] if K == 2 else [0.45, 0.25, 0.15, 0.08, 0.05, 0.02])
    y = rng.choice(K, size=(B, S, S), p=p)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32)
    d.set_class_weights(wc)
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

    def weighted(tn):
        for q in tn.params_list():
            q.grad = None
        logits = tn.forward(x.astype(np.float64), True)
        lg = logits.reshape(-1, K)
        yy = torch.as_tensor(y.reshape(-1), dtype=torch.long)
        ce = F.cross_entropy(lg, yy, reduction="none")
        l2 = sum(0.5 * (w_ ** 2).sum() for w_ in list(tn.w.values()) + list(tn.fcw.values()))
        loss = (torch.as_tensor(wc, dtype=torch.float64)[yy] * ce).sum() / M + WD * l2          # the definition: normalised by the pixel count
        loss.backward()
        return float(loss.detach()), logits.detach().numpy()
    free = TR.TorchNet(net, ch, K, params=params, dtype=torch.float64)
    loss_free, logits_free = weighted(free)
    got_loss = d.loss_value(out["loss_parts"])
    lg = d.logits[:M * K].cpu().numpy().reshape(B, S, S, K)
    assert rel_err(lg, logits_free) < 1e-3
    assert abs(got_loss - loss_free) < 1e-4 * abs(loss_free)
    forced = _ForcedTorchNet(net, ch, K, params=params, dtype=torch.float64)
    forced.dec = dec
    loss_ref, logits_ref = weighted(forced)
    print("weighted step %s: loss %.9g free %.9g forced %.9g" % (net, got_loss, loss_free, loss_ref))
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
    # the unweighted quantities of the same step
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (y.reshape(-1), out["pred"].cpu().numpy().reshape(-1)), 1)
    np.testing.assert_array_equal(out["conf"].cpu().numpy(), cm)
    # an eval forward ignores the weights
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S)
    _, l1 = d.forward(B, S)
    l1 = l1.clone()
    d.set_class_weights(None)
    _, l0 = d.forward(B, S)
    assert torch.equal(l0, l1)


# ------------------------------------------------------------------------------------------------- histogram
def test_label_histogram_equals_bincount(lib):
    from drs_amd import patches as P
    rng = np.random.default_rng(5)
    shapes = [(37, 53), (64, 64), (5, 7), (300, 211)]             # 1961 + 4096 + 35 + 63300 labels: no map a multiple of the 256-thread block
    labs = [rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 255], size=s, p=[0.4, 0.2, 0.1, 0.1, 0.05, 0.03, 0.0, 0.1, 0.02]).astype(np.uint8) for s in shapes]
    pool = P.TilePool([np.zeros(s + (3,), dtype=np.float32) for s in shapes], labs, DEV, dtype=np.float32)
    flat = np.concatenate([l.reshape(-1) for l in labs])
    assert flat.size % 256 and all((s[0] * s[1]) % 256 for s in shapes[:1] + shapes[2:])
    for K, void in ((6, None), (7, 7), (8, None), (8, 7), (2, None), (7, -1), (6, 3)):
        keep = flat[flat != void] if void is not None and void >= 0 else flat
        want = np.bincount(keep, minlength=256)[:K]
        got = pool.label_counts(K, void)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, want)
    # one map alone through the entry point, accumulating over two calls
    one = dev(labs[0].reshape(-1))
    counts = torch.zeros(6, dtype=torch.int64, device=DEV)
    for _ in range(2):
        lib.call("drs_label_histogram", one.data_ptr(), one.numel(), 6, -1, counts.data_ptr(), stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(counts.cpu().numpy(), 2 * np.bincount(labs[0].reshape(-1), minlength=256)[:6])
    assert lib.query("drs_label_histogram", one.data_ptr(), one.numel(), 9, -1, counts.data_ptr(), stream()) == 1


# ------------------------------------------------------------------------------------------------- two ranks
DP = ("dilated8_grsl", 5, 6, 4, 21)


def _dp_inputs():
    rng = np.random.default_rng(0)
    NET, CH, K, B, S = DP
    y = rng.choice(K, size=(B, S * S), p=[0.5, 0.25, 0.12, 0.08, 0.04, 0.01])
    return rng.normal(size=(B, S * S * CH)).astype(np.float32), y


def _dp_weights(y, K, device):
    """what a rank does in the loops: the counts of the (shared) label maps on ITS device, the recipe on the host"""
    from drs_amd import patches as P
    B = y.shape[0]
    S = int(round(np.sqrt(y.shape[1])))
    pool = P.TilePool([np.zeros((S, S, 3), dtype=np.float32)] * B, [y[b].reshape(S, S) for b in range(B)], device, dtype=np.float32)
    counts = pool.label_counts(K)
    return counts, P.check_class_weights(list(P.class_weights(counts, "balanced")), K)


def _dp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from drs_amd.dist import TorchComm, shard_slice
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    torch.cuda.set_device(0)
    comm = TorchComm("gloo")
    x, y = _dp_inputs()
    counts, wc = _dp_weights(y, K, "cuda:0")
    comm.agree([int(c) for c in counts] + [int(v) for v in wc.view(np.uint32)], "class weights")
    sl = shard_slice(B, rank, world)
    d = DilatedNet(NET, CH, K, 0.005, b_max=B // world, s_max=S, device="cuda:0", seed=3, comm=comm)
    d.set_class_weights(wc)
    d.feed(x[sl], y[sl], S)
    res = d.train_step(B // world, S, 0.01)
    torch.cuda.synchronize()
    np.savez(out + "_rank%d.npz" % rank, grads=d.grads.cpu().numpy(), params=d.params.cpu().numpy(), bn=d.bn.cpu().numpy(),
             loss=d.loss_value(res["loss_parts"]), conf=res["conf"].cpu().numpy(), wc=d.class_weights, counts=counts)
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_weighted_step_follows_the_single_rank_step(tmp_path):
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(2, 29600 + os.getpid() % 1000, out), nprocs=2, join=True)
    x, y = _dp_inputs()
    counts, wc = _dp_weights(y, K, DEV)
    d = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=3)
    d.set_class_weights(wc)
    d.feed(x, y, S)
    res = d.train_step(B, S, 0.01)
    torch.cuda.synchronize()
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    # both ranks report identical weights (and counts), the single process's too
    assert r0["wc"].tobytes() == r1["wc"].tobytes() == wc.tobytes() and wc.max() > 5 * wc.min()
    np.testing.assert_array_equal(r0["counts"], r1["counts"])
    np.testing.assert_array_equal(r0["counts"], np.bincount(y.reshape(-1), minlength=K))

    def rel(a, b):
        return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))
    # the bounds of tests/test_gpu_dp.py::test_two_rank_step_equals_single_rank
    assert abs(float(r0["loss"]) - d.loss_value(res["loss_parts"])) < 1e-6
    assert rel(r0["grads"], d.grads.cpu().numpy()) < 2e-3
    assert rel(r0["params"], d.params.cpu().numpy()) < 1e-4
    assert rel(r0["bn"], d.bn.cpu().numpy()) < 1e-6
    np.testing.assert_array_equal(r0["conf"], res["conf"].cpu().numpy())
    np.testing.assert_array_equal(r0["params"], r1["params"])


# ------------------------------------------------------------------------------------------------- loop
def test_train_loop_prints_the_weighted_loss(tmp_path, capsys, monkeypatch):
    from drs_amd import loops, sampling as SP
    from drs_amd.engine import EngineNet
    from drs_amd.synthetic import make_tile
    K, WD = 6, 0.005
    tiles = [make_tile(96, 110, 5, K, seed=1, n_seeds=30), make_tile(80, 96, 5, K, seed=2, n_seeds=30)]
    data, labels = [t[0] for t in tiles], [t[1].copy() for t in tiles]
    for lab in labels:                                       # one rare class: class 5 keeps one corner block (the sampler wants a window of it)
        rare = lab == 5
        lab[rare] = 4
        lab[:18, :18] = 5
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
                      val_cache_dir=str(tmp_path), class_weights="balanced")
    text = capsys.readouterr().out
    counts = np.bincount(np.concatenate([l.reshape(-1) for l in labels]), minlength=K)
    assert "Class weights (balanced): pixel counts " + str([int(c) for c in counts]) in text
    wc = net.class_weights
    want = (counts.sum() / (K * counts.astype(np.float64))).astype(np.float32)
    assert wc.tobytes() == want.tobytes() and wc[5] == wc.max() and wc[5] > 3 * wc.min()
    printed = [float(v) for v in re.findall(r"Training Minibatch: Loss= ([0-9.eE+-]+)", text)]
    assert len(printed) == len(seen) == 4
    for got, (lg, yy, parts) in zip(printed, seen):
        mx = lg.max(axis=1)
        ce = np.log(np.exp(lg - mx[:, None]).sum(axis=1)) + mx - lg[np.arange(len(yy)), yy]
        ref = float((wc.astype(np.float64)[yy] * ce).sum() / len(yy)) + WD * float(parts[1])
        plain = float(ce.mean()) + WD * float(parts[1])
        print("loop loss printed %.6f weighted %.6f unweighted %.6f" % (got, ref, plain))
        assert abs(got - ref) < 1e-4 * min(1.0, abs(ref))
    assert os.path.isfile(out + "class_weights_step_4.npy")
    np.testing.assert_array_equal(np.load(out + "class_weights_step_4.npy"), wc)
    # a resumed run trains the same loss and says so; weights given on a resumed run replace the restored ones, and the log says that too
    args = (data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 5, WD, mean, std, "loss", "single_fixed", [13], None, None, None,
            None, 20, out, 1, "dilated_grsl", "vaihingen", out + "model-4")
    net2 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path))
    text = capsys.readouterr().out
    assert "Class weights (restored from " + out + "class_weights_step_4.npy): weights" in text and net2.class_weights.tobytes() == wc.tobytes()
    net3 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path), class_weights="median")
    text = capsys.readouterr().out
    assert "Class weights (median): pixel counts" in text and "replacing the weights restored from the checkpoint" in text
    f = counts / float(counts.sum())
    assert net3.class_weights.tobytes() == (np.median(f) / f).astype(np.float32).tobytes()
