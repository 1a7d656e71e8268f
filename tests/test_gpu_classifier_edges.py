"""-m gpu: the fused classifier (drs_classifier_loss and its _weighted / _focal twins; vector-ALU, register MFMA and LDS-DMA MFMA form)
on the inputs the Gaussian cases of test_gpu_ops.py / test_gpu_class_weights.py / test_gpu_focal_loss.py never produce:

1. steep logits in the plain and the weighted mode (classifier weights x 48): pixels whose logits pass ln FLT_MAX = 88.7, where exp
   overflows without the max-subtraction, pixels with 1 - p_t < 1e-6 and pixels with p_t < 1e-4; teacher-forced on the device's own
   logits, at the tolerances of test_gpu_focal_loss.py::test_steep_logits_teacher_forced;
2. exact ties in the arg-max: integer logits (features and weights from {-1, 0, 1}, biases from {-1, 0, 1}: every partial sum an
   integer far below 2^24, so every order of summation gives the same bits and fp64 `feat @ w + bias` IS the answer), about a dozen
   live channels, so that every class pair ties for the maximum, three classes tie, and on a few pixels all K do -- numpy's first
   maximum is the rule (tf.argmax);
3. launches with nothing in the loss (loss_mask all zero, every label 255), nothing in the confusion matrix, whole workgroups out of
   the loss, pixel counts 1 / 15 / 16 / 17, and the LDS-DMA form at the product library's own pick on a ragged pixel count.

Every float output is filled with NaN (pred with 255) before the launch: what the kernel leaves unwritten shows.  References are fp64
numpy on the host; what a case is built on (counts of overflowing / confident / wrong pixels, tie counts, bit-equality of the float32
and float64 integer logits) is asserted on the reference alone, in the test."""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

from focal_ref import focal_closed_form   # noqa: E402
from gpu_util import DEV, dev, padded, rel_err, stream   # noqa: E402
from test_gpu_class_weights import WEIGHTS, _case   # noqa: E402  (helpers only: the inputs of the moderate cases, the weights with one exact 0)
from test_gpu_focal_loss import _figures, _reference   # noqa: E402  (helpers only: the fp64 definition and the four figures)


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


def _form(C, K, M):
    """the form the product library picks (csrc/pointwise.hip drs_classifier_loss_focal)"""
    return "valu" if K < 4 else ("dma" if M >= (1 << 18) and C <= 256 else "mfma")


def _check_form(name, shape, exact=True):
    C, K, B, S, P = shape
    M = B * S * S
    assert _form(C, K, M) == name.split("-")[0]
    if name.startswith("dma") and exact:
        assert M == 1 << 18                 # the smallest pixel count that selects it
    return M


ENTRY = {"plain": "drs_classifier_loss", "weighted": "drs_classifier_loss_weighted", "focal": "drs_classifier_loss_focal"}


class _Run(object):
    """one launch of the classifier through `entry` and its slab reductions (the pattern of tests/test_gpu_focal_loss.py::_Run); every
    float output starts as NaN and pred as 255, the confusion matrix (which the kernel ADDS to) as 0; every raw output kept"""

    RAW = ("logits", "pred", "gfeat", "dwp", "dbp", "lp", "conf")
    FLOATS = ("logits", "gfeat", "dwp", "dbp", "lp", "dw", "db", "ls")

    def __init__(self, lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, inv_n, wc=None, gamma=0.0, mode="plain"):
        M = B * S * S
        rows = lib.query("drs_classifier_rows", B, S)
        nan = float("nan")
        self.logits = torch.full((M * K,), nan, dtype=torch.float32, device=DEV)
        self.pred = torch.full((M,), 255, dtype=torch.uint8, device=DEV)
        self.gfeat = torch.full((M * C,), nan, dtype=torch.float32, device=DEV)
        self.dwp = torch.full((rows * C * K,), nan, dtype=torch.float32, device=DEV)
        self.dbp = torch.full((rows * K,), nan, dtype=torch.float32, device=DEV)
        self.lp = torch.full((rows,), nan, dtype=torch.float64, device=DEV)
        self.conf = torch.zeros(K * K, dtype=torch.int32, device=DEV)
        head = (fd.data_ptr(), B, S, P, C, 0, C, K, wdev.data_ptr(), bdev.data_ptr(), yd.data_ptr(), None if lmd is None else lmd.data_ptr(),
                None if amd is None else amd.data_ptr(), inv_n)
        tail = (self.logits.data_ptr(), self.pred.data_ptr(), self.gfeat.data_ptr(), C, 0, self.dwp.data_ptr(), self.dbp.data_ptr(),
                self.lp.data_ptr(), self.conf.data_ptr(), stream())
        self.wc = None if wc is None else np.ascontiguousarray(wc, dtype=np.float32)
        wptr = None if wc is None else self.wc.ctypes.data
        mid = {"plain": (), "weighted": (wptr,), "focal": (wptr, float(gamma))}[mode]
        lib.call(ENTRY[mode], *(head + mid + tail))
        self.dw = torch.full((C * K,), nan, dtype=torch.float32, device=DEV)
        self.db = torch.full((K,), nan, dtype=torch.float32, device=DEV)
        self.ls = torch.full((1,), nan, dtype=torch.float64, device=DEV)
        scr = torch.zeros(lib.query("drs_colsum_scratch_doubles", C * K), dtype=torch.float64, device=DEV)
        lib.call("drs_rows_reduce_f32", self.dwp.data_ptr(), rows, C * K, self.dw.data_ptr(), scr.data_ptr(), stream())
        lib.call("drs_rows_reduce_f32", self.dbp.data_ptr(), rows, K, self.db.data_ptr(), scr.data_ptr(), stream())
        lib.call("drs_sum_f64", self.lp.data_ptr(), rows, self.ls.data_ptr(), stream())
        torch.cuda.synchronize()

    def all_finite(self):
        for name in self.FLOATS:
            assert bool(torch.isfinite(getattr(self, name)).all()), name
        assert int(self.pred.max()) < 255


def _infer(lib, fd, B, S, P, C, K, wdev, bdev):
    """the inference call: labels NULL, pred only"""
    pred = torch.full((B * S * S,), 255, dtype=torch.uint8, device=DEV)
    lib.call("drs_classifier_loss", fd.data_ptr(), B, S, P, C, 0, C, K, wdev.data_ptr(), bdev.data_ptr(), None, None, None, 0.0,
             None, pred.data_ptr(), None, 0, 0, None, None, None, None, stream())
    torch.cuda.synchronize()
    return pred


def _confusion(yy, pred, sel, K):
    cm = np.zeros((K, K), dtype=np.int64)
    sel = sel & (yy < K)
    np.add.at(cm, (yy[sel], pred[sel]), 1)
    return cm


def _inputs(C, K, B, S, seed):
    """Gaussian features, N(0, 1) / sqrt(C) weights, uniform labels with about 1 % at 255, 70 % of the pixels in the loss, 80 % in the
    confusion matrix -- for the class counts tests/test_gpu_class_weights.py::_case has no table entry for"""
    rng = np.random.default_rng(seed)
    feat = rng.standard_normal(size=(B, S, S, C), dtype=np.float32)
    w = (rng.normal(size=(C, K)) / np.sqrt(C)).astype(np.float32)
    bias = (rng.normal(size=K) * 0.1).astype(np.float32)
    y = rng.integers(0, K, size=(B, S, S)).astype(np.uint8)
    y[rng.random(size=y.shape) < 0.01] = 255
    lm = (rng.random(size=y.shape) < 0.7).astype(np.uint8)
    am = (rng.random(size=y.shape) < 0.8).astype(np.uint8)
    return feat, w, bias, y, lm, am


def _against_fp64(r, feat, w, bias, y, lm, am, n, wc, gamma, what, few_pixels=False):
    """a launch `r` (inv_n = 1 / n) against fp64 numpy at the tolerances of tests/test_gpu_class_weights.py / test_gpu_focal_loss.py:
    logits and gradients 1e-5 of the tensor's maximum, loss 1e-6 relative, arg-max the first maximum of the device's own logits,
    confusion matrix exact, exact zeros outside the loss.  lm / am: [M] or None.  Returns the in-loss selection.
    few_pixels: the loss at the bound of tests/test_gpu_ops.py::test_classifier_loss, 1e-5 max(1, |L|) absolute -- a pixel's CE is
    log se + max - logit_y in fp32, three roundings at the size of the logits (~ 1e-7 absolute) whatever the size of the CE; the
    relative 1e-6 rests on hundreds of such terms averaging, which a sum over 1 to 16 pixels does not do."""
    K = w.shape[1]
    C = w.shape[0]
    M = y.size
    f64, w64 = feat.reshape(M, C).astype(np.float64), w.astype(np.float64)
    lg_ref = f64 @ w64 + bias.astype(np.float64)
    yy = y.reshape(-1).astype(np.int64)
    inl = (yy < K) & (np.ones(M, dtype=bool) if lm is None else lm.reshape(-1) > 0)
    r.all_finite()
    lg = r.logits.cpu().numpy().reshape(M, K)
    assert rel_err(lg, lg_ref) < 1e-5
    ph = r.pred.cpu().numpy()
    np.testing.assert_array_equal(ph, lg.argmax(axis=1))
    np.testing.assert_array_equal(r.conf.cpu().numpy().reshape(K, K), _confusion(yy, ph, np.ones(M, dtype=bool) if am is None else am.reshape(-1) > 0, K))
    wc = np.ones(K, dtype=np.float32) if wc is None else np.asarray(wc, dtype=np.float32)
    loss_ref, gl, _ = _reference(lg_ref, yy, inl, wc, gamma, n, K)
    figures = _figures(r, dict(n=n, f64=f64, w64=w64), loss_ref, gl, M, C, K)
    print("%s: %s" % (what, figures))
    assert not r.gfeat.view(M, C)[torch.from_numpy(~inl).to(DEV)].any()
    if few_pixels:
        assert figures["loss"] * abs(loss_ref) < 1e-5 * max(1.0, abs(loss_ref))
    else:
        assert figures["loss"] < 1e-6
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5
    return inl


# ------------------------------------------------------------------------------------------------- 1. steep logits
# Classifier weights x 48, chosen on the CPU from the fp64 reference alone (seeds of the focal steep test): in-loss pixels with
# max|logit| > 89 / q < 1e-6 / p_t < 1e-4: 37 / 87 / 125 of M = 338 at valu-K2, 309 / 110 / 721 of M = 1323 at mfma-K6,
# 57086 / 20254 / 140054 of M = 2^18 at the LDS-DMA form; x 32 leaves 6 pixels past 89 at valu-K2 -- too few.
STEEP_SCALE = 48.0
LN_FLT_MAX = 89.0         # past ln FLT_MAX = 88.72: exp of such a logit is inf in fp32
# (the large form first: the cached inputs the module leaves behind are then the small ones)
STEEP_FORMS = {"dma-K6-64x64x64": (256, 6, 64, 64, 0), "valu-K2": (448, 2, 2, 13, 6), "mfma-K6": (256, 6, 3, 21, 0)}
STEEP = [(f, m) for f in STEEP_FORMS for m in ("plain", "weighted")]


@functools.lru_cache(maxsize=1)
def _steep_inputs(form):
    """the inputs of a form with the weights scaled, on the host in fp64 and on the device: computed once, shared by the two modes, left unchanged"""
    C, K, B, S, P = STEEP_FORMS[form]
    M = B * S * S
    feat, w, bias, y, lm, am = _case(C, K, B, S, seed=3 * C + K)
    w = (w * STEEP_SCALE).astype(np.float32)
    d = dict(fd=padded(feat, P, fill=3.0) if P else dev(feat), yd=dev(y.reshape(-1)), amd=dev(am.reshape(-1)), lmd=dev(lm.reshape(-1)),
             wdev=dev(w), bdev=dev(bias), n=float(lm.sum()))
    d["f64"] = feat.reshape(M, C).astype(np.float64)
    d["w64"] = w.astype(np.float64)
    d["lg_ref"] = d["f64"] @ d["w64"] + bias.astype(np.float64)
    d["yy"] = y.reshape(-1).astype(np.int64)
    d["inl"] = (d["yy"] < K) & (lm.reshape(-1) > 0)
    return d


def _regimes(lg, yy, inl, wc, K):
    """in-loss pixels whose largest |logit| overflows exp, that are confident (q = 1 - p_t < 1e-6), that are wrong (p_t < 1e-4)"""
    ref = focal_closed_form(lg, np.minimum(yy, K - 1), wc.astype(np.float64), 0.0)
    return int((inl & (np.abs(lg).max(axis=1) > LN_FLT_MAX)).sum()), int((inl & (ref["q"] < 1e-6)).sum()), int((inl & (ref["pt"] < 1e-4)).sum())


@pytest.mark.parametrize("form,mode", STEEP, ids=["%s-%s" % fm for fm in STEEP])
def test_steep_logits_plain_and_weighted_teacher_forced(lib, form, mode):
    """fp32 rounding of logits this large is not the subject: the fp64 softmax-CE and its logit gradient are evaluated on the DEVICE'S
    OWN logits.  Without the max-subtraction exp overflows on the first group of pixels; a maximum that is wrong in one of a pixel's
    four lanes, or a log se + max - logit_y that loses the label's logit, shows in the loss and the gradients of the other two."""
    C, K, B, S, P = STEEP_FORMS[form]
    M = _check_form(form, STEEP_FORMS[form])
    d = _steep_inputs(form)
    yy, inl, n = d["yy"], d["inl"], d["n"]
    weights = np.asarray(WEIGHTS[K], dtype=np.float32)          # unequal, one exact 0
    wc = weights if mode == "weighted" else np.ones(K, dtype=np.float32)
    # the reference alone shows the three regimes, about 1 % of the labels at 255, and a loss mask that is neither empty nor full
    counts = _regimes(d["lg_ref"], yy, inl, wc, K)
    print("steep %s %s: in-loss pixels with max|logit| > 89: %d, with q < 1e-6: %d, with p_t < 1e-4: %d" % ((form, mode) + counts))
    assert min(counts) > 10
    assert 0.005 * M < (yy == 255).sum() < 0.03 * M and 10 < n < M - 10
    r = _Run(lib, d["fd"], B, S, P, C, K, d["wdev"], d["bdev"], d["yd"], d["lmd"], d["amd"], 1.0 / n, weights if mode == "weighted" else None, 0.0, mode)
    r.all_finite()
    lg = r.logits.cpu().numpy().astype(np.float64).reshape(M, K)
    assert rel_err(lg, d["lg_ref"]) < 1e-5
    np.testing.assert_array_equal(r.pred.cpu().numpy(), lg.argmax(axis=1))          # numpy's arg-max: the first maximum
    assert min(_regimes(lg, yy, inl, wc, K)) > 10
    loss_ref, gl, ref = _reference(lg, yy, inl, wc, 0.0, n, K)
    figures = _figures(r, d, loss_ref, gl, M, C, K)
    print("steep classifier %s %s: %s" % (form, mode, figures))
    # exact zeros: pixels out of the loss, and in the weighted mode the pixels of the class whose weight is 0
    zero = int(np.flatnonzero(weights == 0)[0])
    off = ~inl | (yy == zero) if mode == "weighted" else ~inl
    assert (weights == 0).sum() == 1 and (inl & (yy == zero)).sum() > 10 and (~inl).sum() > 10
    assert not r.gfeat.view(M, C)[torch.from_numpy(off).to(DEV)].any()
    assert bool(r.gfeat.view(M, C)[torch.from_numpy(inl & (yy != zero) & (ref["q"] > 1e-3)).to(DEV)].any(dim=1).all())
    assert figures["loss"] < 1e-6
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5


# ------------------------------------------------------------------------------------------------- 2. exact ties
TIE_FORMS = {"valu-K2": (448, 2, 2, 13, 6), "valu-K3": (192, 3, 2, 15, 1), "mfma-K6": (256, 6, 3, 21, 0), "dma-K4-64x64x64": (64, 4, 64, 64, 0)}
TIE_LIVE = 12         # live channels: dense +-1 weights spread the logits too far (least-tied pair 2 pixels at (256, 6, 3, 21)); a dozen give sigma ~ 2


def _tie_case(C, K, B, S, seed):
    """Integer logits.  Features from {-1, 0, 1}; weights from {-1, 0, 1} on TIE_LIVE channels, 0 on the others; biases a permutation
    of 1, -1, 0, 1, ... (unequal).  One live channel d carries the weight row -bias, and a block of 8 pixels has channel d at 1 and
    every other live channel at 0: all K logits of those pixels are 0."""
    rng = np.random.default_rng(seed)
    M = B * S * S
    feat = rng.integers(-1, 2, size=(M, C)).astype(np.float32)
    live = rng.choice(C, size=TIE_LIVE, replace=False)
    w = np.zeros((C, K), dtype=np.float32)
    w[live] = rng.integers(-1, 2, size=(TIE_LIVE, K))
    bias = rng.permutation(np.resize(np.asarray([1, -1, 0], dtype=np.float32), K))
    w[live[0]] = -bias
    n_eq = min(8, M)
    blk = np.arange(M // 3, M // 3 + n_eq)
    feat[np.ix_(blk, live)] = 0.0
    feat[blk, live[0]] = 1.0
    y = rng.integers(0, K, size=M).astype(np.uint8)
    lm = rng.integers(0, 2, size=M).astype(np.uint8)
    am = rng.integers(0, 2, size=M).astype(np.uint8)
    return feat.reshape(B, S, S, C), w, bias, y, lm, am


def _exact_logits_and_ties(feat, w, bias, what):
    """the exact logits (fp64) of an integer case; asserts what the case is built on, on the reference alone"""
    C, K = w.shape
    f32 = feat.reshape(-1, C)
    lg_ref = f32.astype(np.float64) @ w.astype(np.float64) + bias.astype(np.float64)
    # every partial sum, in any order, is an integer of magnitude <= sum |f| |w| + |b| < 2^24: exact in fp32 ...
    assert float((np.abs(f32) @ np.abs(w)).max() + np.abs(bias).max()) < 2 ** 24 and np.array_equal(lg_ref, np.rint(lg_ref))
    # ... and the float32 product is the float64 product bit for bit
    lg32 = f32 @ w + bias
    assert lg32.dtype == np.float32 and lg32.tobytes() == lg_ref.astype(np.float32).tobytes() and np.array_equal(lg32.astype(np.float64), lg_ref)
    top = lg_ref == lg_ref.max(axis=1, keepdims=True)
    pairs = {(i, j): int((top[:, i] & top[:, j]).sum()) for i, j in itertools.combinations(range(K), 2)}
    three, every = int((top.sum(axis=1) >= 3).sum()), int(top.all(axis=1).sum())
    print("ties %s: least-tied class pair %d pixels, most-tied %d, three-way or more %d, all %d classes equal %d (of %d pixels, logit sigma %.2f)"
          % (what, min(pairs.values()), max(pairs.values()), three, K, every, lg_ref.shape[0], lg_ref.std()))
    assert min(pairs.values()) >= 10 and (K < 3 or three >= 10) and every >= 1
    return lg_ref


@pytest.mark.parametrize("form", list(TIE_FORMS))
def test_argmax_takes_the_first_maximum_on_exact_ties(lib, form):
    C, K, B, S, P = TIE_FORMS[form]
    M = _check_form(form, TIE_FORMS[form])
    feat, w, bias, y, lm, am = _tie_case(C, K, B, S, seed=C + K + S)
    lg_ref = _exact_logits_and_ties(feat, w, bias, form)
    fd = padded(feat, P, fill=3.0) if P else dev(feat)
    wdev, bdev = dev(w), dev(bias)
    n = float(lm.sum())
    r = _Run(lib, fd, B, S, P, C, K, wdev, bdev, dev(y), dev(lm), dev(am), 1.0 / n)
    r.all_finite()
    assert r.logits.cpu().numpy().tobytes() == lg_ref.astype(np.float32).tobytes()            # bit for bit
    ph = r.pred.cpu().numpy()
    want = lg_ref.argmax(axis=1)                  # numpy's arg-max: the first maximum
    np.testing.assert_array_equal(ph, want)
    yy = y.astype(np.int64)
    np.testing.assert_array_equal(r.conf.cpu().numpy().reshape(K, K), _confusion(yy, want, am > 0, K))
    np.testing.assert_array_equal(_infer(lib, fd, B, S, P, C, K, wdev, bdev).cpu().numpy(), want)
    # loss and gradients: the tolerances of tests/test_gpu_ops.py::test_classifier_loss
    f64, w64 = feat.reshape(M, C).astype(np.float64), w.astype(np.float64)
    ce, gl = T.softmax_ce(lg_ref, y, lm)
    assert abs(r.ls.item() / n - ce) < 1e-5 * max(1.0, abs(ce))
    assert rel_err(r.gfeat.cpu().numpy().reshape(M, C), gl @ w64.T) < 2e-5
    assert rel_err(r.dw.cpu().numpy().reshape(C, K), f64.T @ gl) < 2e-5
    assert np.abs(r.db.cpu().numpy() - gl.sum(axis=0)).max() < 2e-6 * np.abs(gl).sum(axis=0).max()


@pytest.mark.parametrize("C,K,B,S,P", [(256, 6, 3, 21, 0), (128, 4, 2, 17, 2)])
def test_forced_forms_agree_bitwise_on_exact_ties(lib, C, K, B, S, P):
    """the vector-ALU (0), register MFMA (2) and LDS-DMA MFMA (3) form of the development library on integer logits: the same logits,
    arg-max and confusion matrix bit for bit, ragged last tiles (M = 1323, 578) and a haloed slab included"""
    lib = lib.dev()
    M = B * S * S
    assert M % 16 and M % 64
    feat, w, bias, y, lm, am = _tie_case(C, K, B, S, seed=C * 3 + K + S)
    lg_ref = _exact_logits_and_ties(feat, w, bias, "forced forms %s" % ((C, K, B, S, P),))
    want = lg_ref.argmax(axis=1)
    fd = padded(feat, P, fill=3.0) if P else dev(feat)
    wdev, bdev, yd, lmd, amd = dev(w), dev(bias), dev(y), dev(lm), dev(am)
    res = {}
    try:
        for v in (0, 2, 3):
            lib.drs_debug_cls_variant(v)
            r = _Run(lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, 1.0 / float(lm.sum()))
            res[v] = (r, _infer(lib, fd, B, S, P, C, K, wdev, bdev))
    finally:
        lib.drs_debug_cls_variant(1)
    cm = _confusion(y.astype(np.int64), want, am > 0, K)
    for v, (r, pred2) in res.items():
        r.all_finite()
        assert r.logits.cpu().numpy().tobytes() == lg_ref.astype(np.float32).tobytes(), v
        np.testing.assert_array_equal(r.pred.cpu().numpy(), want, err_msg=str(v))
        np.testing.assert_array_equal(pred2.cpu().numpy(), want, err_msg=str(v))
        np.testing.assert_array_equal(r.conf.cpu().numpy().reshape(K, K), cm, err_msg=str(v))
        for name in ("logits", "pred", "conf"):
            assert torch.equal(getattr(r, name), getattr(res[0][0], name)), (name, v)
    for name in _Run.RAW + ("dw", "db", "ls"):                  # the two MFMA forms run the same products in the same order
        assert torch.equal(getattr(res[2][0], name), getattr(res[3][0], name)), name


# ------------------------------------------------------------------------------------------------- 3. nothing in the loss, tiny and ragged counts
EMPTY_FORMS = {"valu-K3": (192, 3, 2, 15, 1), "mfma-K6": (256, 6, 3, 21, 0)}
EMPTY_MODES = {"plain": (None, 0.0), "focal": (True, 2.0)}          # focal: gamma = 2 with the class weights
EMPTY = [(f, m, c) for f in EMPTY_FORMS for m in EMPTY_MODES for c in ("a-lossmask0", "b-labels255", "c-accmask0", "d-firsthalf0")]


@pytest.mark.parametrize("form,mode,case", EMPTY, ids=["-".join(e) for e in EMPTY])
def test_nothing_in_the_loss_or_in_the_confusion_matrix(lib, form, mode, case):
    """inv_n = 1.0 (what a caller passes matters to nothing when no pixel is in the loss: no division by a count happens in the kernel).
    (a) loss_mask all zero, (b) every label 255: gradients, their slabs and the loss partials exact zeros, nothing NaN, logits and
    arg-max those of a normal launch; (c) acc_mask all zero, (d) the first half of the pixels out of the loss -- at 64 pixels per
    workgroup whole workgroups see no pixel in the loss: loss and gradients against fp64."""
    C, K, B, S, P = EMPTY_FORMS[form]
    M = _check_form(form, EMPTY_FORMS[form])
    feat, w, bias, y, lm, am = _case(C, K, B, S, seed=C + K + S)
    y, lm, am = y.reshape(-1), lm.reshape(-1), am.reshape(-1)
    wc = np.asarray(WEIGHTS[K], dtype=np.float32) if EMPTY_MODES[mode][0] else None
    gamma = EMPTY_MODES[mode][1]
    fd = padded(feat, P, fill=3.0) if P else dev(feat)
    wdev, bdev = dev(w), dev(bias)
    normal = _Run(lib, fd, B, S, P, C, K, wdev, bdev, dev(y), dev(lm), dev(am), 1.0, wc, gamma, mode)
    normal.all_finite()
    assert float(normal.gfeat.abs().max()) > 0 and float(normal.ls.item()) > 0 and int(normal.conf.sum()) > 0
    if case[0] == "a":
        lm = np.zeros_like(lm)
    elif case[0] == "b":
        y = np.full_like(y, 255)
    elif case[0] == "c":
        am = np.zeros_like(am)
    else:
        lm = lm.copy()
        lm[:M // 2] = 0
        assert M // 2 >= 3 * 64 and lm[M // 2:].sum() > 10           # (drs_classifier_rows: 64 pixels per workgroup at these sizes)
    r = _Run(lib, fd, B, S, P, C, K, wdev, bdev, dev(y), dev(lm), dev(am), 1.0, wc, gamma, mode)
    assert torch.equal(r.logits, normal.logits) and torch.equal(r.pred, normal.pred)
    yy = y.astype(np.int64)
    if case[0] in "ab":
        r.all_finite()
        for name in ("gfeat", "dwp", "dbp", "lp", "dw", "db", "ls"):
            assert not getattr(r, name).any(), name                # exact zeros (a NaN is not zero)
        cm = _confusion(yy, r.pred.cpu().numpy(), am > 0, K)
        assert (cm.sum() == 0) == (case[0] == "b")
        np.testing.assert_array_equal(r.conf.cpu().numpy().reshape(K, K), cm)
        return
    inl = _against_fp64(r, feat, w, bias, y, lm, am, 1.0, wc, gamma, "empty %s %s %s" % (form, mode, case))
    if case[0] == "c":
        assert not r.conf.any() and inl.sum() > 10
    else:
        assert not inl[:M // 2].any() and not r.gfeat.view(M, C)[:M // 2].any()


@pytest.mark.parametrize("B,S", [(1, 1), (15, 1), (1, 4), (17, 1)], ids=["M1", "M15", "M16", "M17"])
@pytest.mark.parametrize("C,K,P", [(128, 6, 0), (64, 2, 1)], ids=["mfma-K6-C128", "valu-K2-C64"])
def test_tiny_pixel_counts(lib, C, K, P, B, S):
    """one pixel, one short of a 16-pixel tile, one tile exactly, one tile and a pixel: the plain and the focal mode against fp64"""
    M = B * S * S
    assert _form(C, K, M) == ("mfma" if K == 6 else "valu")
    rng = np.random.default_rng(C + K + M)
    feat = rng.standard_normal(size=(B, S, S, C), dtype=np.float32)
    w = (rng.normal(size=(C, K)) / np.sqrt(C)).astype(np.float32)
    bias = (rng.normal(size=K) * 0.1).astype(np.float32)
    y = rng.integers(0, K, size=M).astype(np.uint8)
    lm, am = np.ones(M, dtype=np.uint8), np.ones(M, dtype=np.uint8)
    if M > 1:                       # the last pixel out of the loss, the first out of the confusion matrix, one label outside [0, K)
        lm[-1], am[0], y[M // 2] = 0, 0, 255
    n = float(((y < K) & (lm > 0)).sum())
    assert n >= 1
    fd = padded(feat, P, fill=3.0) if P else dev(feat)
    wdev, bdev, yd, lmd, amd = dev(w), dev(bias), dev(y), dev(lm), dev(am)
    for mode, (weighted, gamma) in EMPTY_MODES.items():
        wc = np.asarray(WEIGHTS[K], dtype=np.float32)[::-1].copy() + 0.25 if weighted else None         # (no weight 0: one pixel must still give a loss)
        r = _Run(lib, fd, B, S, P, C, K, wdev, bdev, yd, lmd, amd, 1.0 / n, wc, gamma, mode)
        _against_fp64(r, feat, w, bias, y, lm, am, n, wc, gamma, "tiny C=%d K=%d M=%d %s" % (C, K, M, mode), few_pixels=True)
        np.testing.assert_array_equal(_infer(lib, fd, B, S, P, C, K, wdev, bdev).cpu().numpy(), r.pred.cpu().numpy())


def test_lds_dma_form_at_its_own_pick_on_a_ragged_pixel_count(lib):
    """the product library picks the LDS-DMA form from 2^18 pixels: here M = 4 x 257 x 257 = 264196 = 16 x 16512 + 4 in a haloed slab --
    a last tile of 4 pixels, workgroups past the end of the pixels, slab rows beyond the launch"""
    C, K, B, S, P = 64, 4, 4, 257, 1
    M = _check_form("dma-K4-ragged", (C, K, B, S, P), exact=False)
    assert M >= 1 << 18 and M % 16 == 4
    feat, w, bias, y, lm, am = _inputs(C, K, B, S, seed=C + K + S)
    fd = padded(feat, P, fill=3.0)
    wdev, bdev = dev(w), dev(bias)
    y, lm, am = y.reshape(-1), lm.reshape(-1), am.reshape(-1)
    y[-4:], lm[-4:], am[-4:] = [0, 1, 2, 3], 1, 1              # the four pixels of the last tile: in the loss and in the confusion matrix
    n = float(lm.sum())
    r = _Run(lib, fd, B, S, P, C, K, wdev, bdev, dev(y), dev(lm), dev(am), 1.0 / n)
    inl = _against_fp64(r, feat, w, bias, y, lm, am, n, None, 0.0, "ragged LDS-DMA M=%d" % M)
    assert inl[-4:].all() and 0.005 * M < (y == 255).sum() < 0.02 * M
    np.testing.assert_array_equal(_infer(lib, fd, B, S, P, C, K, wdev, bdev).cpu().numpy(), r.pred.cpu().numpy())
