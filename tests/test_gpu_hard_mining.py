"""-m gpu: online hard example mining in the training loss from the kernel up: the keys of drs_patch_hard_weight against
fp64, its selection bit for bit against the numpy statement (tests/hard_mining_ref.py, itself held by tests/test_hard_mining_plan.py)
on its own keys and on adversarial ones, the pixel map input, containment, a whole training step against fp64 autograd, engine = op
level, the option off, the shared inference launch, two ranks, the training loop and the three command lines.

Rule held here: per patch, the k_b = min(n_b, max(ceil(keep n_b), min_keep)) in-loss pixels with the largest plain cross-entropy are
kept, ties towards the lower pixel index, each at the weight float32(n_b / k_b) times the incoming map; every other pixel gets 0.
Tolerances: the keys 2^-20 (1 + ce) (derived at test_keys_and_selection...), the selection exact, whole nets the project's existing
ones (tests/test_gpu_dice_loss.py: loss and gradients 1e-4, logits 1e-3), two ranks: equal maps, the loss as tests/test_gpu_dp.py,
gradients and parameters that test's bounds times n_b / k_b (reasoned at the test)."""
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import boundary_weight_ref as BR   # noqa: E402
import hard_mining_ref as HR   # noqa: E402
from gpu_util import DEV, dev, rel_err, stream   # noqa: E402
from test_gpu_class_weights import WEIGHTS, _feed_step, _ForcedTorchNet   # noqa: E402  (helpers only)
from test_gpu_dice_loss import BW, DICE, STEP_CASES, _dp_inputs, _step_inputs, _torch_dice   # noqa: E402  (helpers only: the step cases and inputs)


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# ------------------------------------------------------------------------------------------------- the kernel
# 17^2 = 289: more than one pixel per thread, no multiple of 64; 64^2: the headline patch; 65^2: a ragged tail
SHAPES = [(1, 1, 1), (3, 3, 2), (2, 17, 6), (2, 64, 6), (1, 65, 8)]
IDS = ["%dx%dx%d-K%d" % (b, s, s, k) for b, s, k in SHAPES]
KEEPS = [1.0 / 4096, 0.25, 0.5, 1.0]
MIN_KEEPS = [0, 1, 300]
MARK = -7.0


def _launch(lib, B, S, K, keep, min_keep, y, lm, logits=None, ce_in=None, w_in=None, in_place=False, guard=0, want_kept=True):
    """one launch on device tensors -> (ce, w, kept) tensors with `guard` marker elements on either side of each"""
    n, g = B * S * S, guard
    ce = torch.full((n + 2 * g,), MARK, dtype=torch.float32, device=DEV)
    if ce_in is not None:
        ce[g:g + n] = ce_in
    w = torch.full((n + 2 * g,), MARK, dtype=torch.float32, device=DEV)
    if in_place:
        w[g:g + n] = w_in
    kept = torch.full((B + 2 * g,), int(MARK), dtype=torch.int32, device=DEV)
    lib.call("drs_patch_hard_weight", None if logits is None else logits.data_ptr(), ce[g:].data_ptr(), y.data_ptr(),
             None if lm is None else lm.data_ptr(), B, S, K, float(keep), int(min_keep),
             w[g:].data_ptr() if in_place else (None if w_in is None else w_in.data_ptr()), w[g:].data_ptr(),
             kept[g:].data_ptr() if want_kept else None, stream())
    torch.cuda.synchronize()
    return ce, w, kept


def _labels_and_mask(rng, B, n, K):
    """labels with about 5 % >= K scattered in, a loss mask with holes, and (B > 1) a last patch with no pixel in the loss"""
    y = rng.integers(0, K, size=(B, n)).astype(np.uint8)
    out = rng.random(size=y.shape) < 0.05
    y[out] = rng.choice([K, 255], size=int(out.sum())).astype(np.uint8)
    lm = (rng.random(size=y.shape) < 0.7).astype(np.uint8)
    if n > 1:
        lm[0, 0], y[0, 0] = 1, 0
    if B > 1:
        lm[B - 1] = 0
    return y, lm


def _logit_sets(rng, B, n, K, y):
    """name -> logits float32 [B, n, K]: moderate; steep (cross-entropies in the thousands); confident (most keys exactly +0)"""
    base = rng.normal(size=(B, n, K)).astype(np.float32)
    conf = base.copy()
    sure = rng.random(size=(B, n)) < 0.8
    bi, pi = np.nonzero(sure)
    conf[bi, pi, np.minimum(y[bi, pi], K - 1)] += 60.0
    return {"moderate": base * 3.0, "steep": base * 2000.0, "confident": conf}


@pytest.mark.parametrize("B,S,K", SHAPES, ids=IDS)
def test_keys_against_fp64_and_selection_bit_exact_on_its_own_keys(lib, B, S, K):
    """(1) ce against fp64 from the same logits within 2^-20 (1 + ce64): se is a sum of K <= 8 fp32 terms of <= 2-ulp expf, logf has
    <= 2 ulp, one rounding each in max - logit_y and in the final add: under 16 2^-24 + 4 2^-24 ce, the bound leaves 4x.  (2) weight_out
    and kept_out are the reference selection applied to the kernel's OWN keys, bit for bit."""
    rng = np.random.default_rng(100 * S + K)
    n = S * S
    y, lm = _labels_and_mask(rng, B, n, K)
    yd, lmd = dev(y.reshape(-1)), dev(lm.reshape(-1))
    worst = 0.0
    for name, lg in _logit_sets(rng, B, n, K, y).items():
        lgd = dev(lg.reshape(-1))
        for mask, maskd in ((lm, lmd), (None, None)):
            inl = HR.in_loss(y, K, mask)
            ce64 = np.where(inl, HR.cross_entropy(lg.astype(np.float64), np.minimum(y, K - 1)), 0.0)
            if n >= 289:
                if name == "steep":
                    assert ce64.max() > 1000.0
                if name == "confident":
                    assert (ce64[inl] < 1e-20).sum() > 0.5 * inl.sum()
            for keep in KEEPS:
                for min_keep in MIN_KEEPS:
                    ce, w, kept = _launch(lib, B, S, K, keep, min_keep, yd, maskd, logits=lgd)
                    ce, w, kept = ce.cpu().numpy().reshape(B, n), w.cpu().numpy().reshape(B, n), kept.cpu().numpy()
                    err = np.abs(ce.astype(np.float64) - ce64) / (1.0 + ce64)
                    worst = max(worst, float(err[inl].max()) if inl.any() else 0.0)
                    assert (err[inl] <= 2.0 ** -20).all(), (name, keep, min_keep, float(err[inl].max()))
                    assert (ce.view(np.uint32)[~inl] == 0).all()                         # exactly +0 outside the loss
                    assert not np.signbit(ce).any() and not np.isnan(ce).any()
                    if name == "confident" and n >= 289:
                        assert (ce.view(np.uint32)[inl] == 0).sum() > 0.5 * inl.sum()    # many keys exactly +0: ties at the bottom
                    want_w, want_k = HR.weights(ce, inl, keep, min_keep)
                    np.testing.assert_array_equal(kept, want_k, err_msg="%s keep %g min_keep %d" % (name, keep, min_keep))
                    np.testing.assert_array_equal(w.view(np.uint32), want_w.view(np.uint32), err_msg="%s keep %g min_keep %d" % (name, keep, min_keep))
                    assert ((w != 0).sum(axis=1) == want_k).all()
    print("hard-mining keys %dx%dx%d K%d: worst |ce - ce64| / (1 + ce64) = %.3g (bound %.3g)" % (B, S, S, K, worst, 2.0 ** -20))


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _key_sets(rng, B, n):
    """name -> keys float32 [B, n], all >= +0 and not NaN"""
    one = np.float32(1.0).view(np.uint32)
    sets = {
        "all-equal": np.full((B, n), 0.75, dtype=np.float32),                                        # only the tie rule decides
        "adjacent-floats": _f32(one + rng.integers(0, 4, size=(B, n)).astype(np.uint32)),            # the last radix pass decides
        "low-bytes-only": _f32(one + rng.integers(0, 1 << 16, size=(B, n)).astype(np.uint32)),       # the last two passes decide
        "few-values": rng.choice(np.asarray([0.5, 1.0, 2.0], dtype=np.float32), size=(B, n)),        # ties across threads and waves at the threshold
        "ramp-up": np.tile(np.arange(n, dtype=np.float32) / 1024.0, (B, 1)),
        "ramp-down": np.tile(np.arange(n, dtype=np.float32)[::-1] / 1024.0, (B, 1)),
        "random-bits": _f32(rng.integers(0, 0x7F800000, size=(B, n), dtype=np.int64).astype(np.uint32)),   # every exponent
    }
    special = rng.random(size=(B, n)).astype(np.float32)
    kind = rng.integers(0, 5, size=(B, n))
    special[kind == 0] = _f32(rng.integers(1, 100, size=int((kind == 0).sum())).astype(np.uint32))    # denormals
    special[kind == 1] = 0.0
    special[kind == 2] = np.inf
    sets["denormals-zero-inf"] = special
    return sets


@pytest.mark.parametrize("B,S,K", SHAPES, ids=IDS)
def test_selection_on_adversarial_keys_bit_exact(lib, B, S, K):
    """(3) logits = NULL, ce as input: the selection alone, against the reference, on keys chosen to break a radix select or a tie rule"""
    rng = np.random.default_rng(7 * S + K)
    n = S * S
    y, lm = _labels_and_mask(rng, B, n, K)
    full = np.zeros_like(y)                            # every pixel in the loss ...
    lm_pair = np.ones_like(lm)
    if B > 1:
        lm_pair[0] = 0                                 # ... and a patch wholly outside the loss next to a full one
    layouts = {"mask+labels>=K": (y, lm), "no-mask": (y, None), "all-in": (full, None), "empty-beside-full": (full, lm_pair)}
    ties_seen = 0
    for lname, (yy, mask) in layouts.items():
        yd, maskd = dev(yy.reshape(-1)), None if mask is None else dev(mask.reshape(-1))
        inl = HR.in_loss(yy, K, mask)
        for kname, keys in _key_sets(rng, B, n).items():
            given = np.where(inl, keys, np.float32(np.inf))        # entries outside the loss are not read: were they, +inf would be kept first
            for keep in KEEPS:
                for min_keep in MIN_KEEPS:
                    want_w, want_k = HR.weights(keys, inl, keep, min_keep)
                    ce, w, kept = _launch(lib, B, S, K, keep, min_keep, yd, maskd, ce_in=dev(given.reshape(-1)))
                    what = "%s %s keep %g min_keep %d" % (lname, kname, keep, min_keep)
                    np.testing.assert_array_equal(kept.cpu().numpy(), want_k, err_msg=what)
                    np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32).reshape(B, n), want_w.view(np.uint32), err_msg=what)
                    assert torch.equal(ce, dev(given.reshape(-1)))                                   # the input is left as it came
                    for b in range(B):                 # the k_b-th and (k_b + 1)-th keys equal: the tie rule decided this case
                        s = np.sort(keys[b][inl[b]])[::-1]
                        if 0 < want_k[b] < s.size and s[want_k[b] - 1] == s[want_k[b]]:
                            ties_seen += 1
    assert n < 4 or ties_seen > 20, ties_seen


def test_ties_span_thread_and_wave_borders(lib):
    """the k_b-th and (k_b + 1)-th keys equal, the tied run placed across a wave border (pixel 63 | 64), a round border (255 | 256) and
    the ragged tail of 65^2 = 4225 = 16 * 256 + 129"""
    B, S, K = 1, 65, 8
    n = S * S
    y = dev(np.zeros(n, dtype=np.uint8))
    for first, count, take in ((60, 10, 5), (250, 12, 7), (4090, 135, 130), (0, n, 1000), (62, 2, 1), (255, 2, 1)):
        keys = np.full((1, n), 0.25, dtype=np.float32)
        keys[0, first:first + count] = 1.0             # the tied run ...
        above = np.asarray([5, 2000, 4100][:2]) if first > 10 else np.asarray([], dtype=np.int64)
        above = above[(above < first) | (above >= first + count)]
        keys[0, above] = 3.0                           # ... below a few larger keys
        k = above.size + take
        want_w, want_k = HR.weights(keys, np.ones((1, n), dtype=bool), 1e-9, k)
        assert want_k[0] == k and np.flatnonzero(want_w[0]).tolist() == sorted(above.tolist() + list(range(first, first + take)))
        _, w, kept = _launch(lib, B, S, K, 1e-9, k, y, None, ce_in=dev(keys.reshape(-1)))
        assert int(kept[0]) == k
        np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), want_w.reshape(-1).view(np.uint32), err_msg=str((first, count, take)))


@pytest.mark.parametrize("B,S,K", SHAPES[1:], ids=IDS[1:])
def test_pixel_map_input_separate_and_in_place(lib, B, S, K):
    """(4) with pixel_weight_in the result is float32(n_b / k_b) * w_in, one fp32 multiply, bit for bit; with k_b = n_b the map is
    returned unchanged bit for bit (0 outside the loss, where no pixel is kept)"""
    rng = np.random.default_rng(S)
    n = S * S
    y, lm = _labels_and_mask(rng, B, n, K)
    yd, lmd = dev(y.reshape(-1)), dev(lm.reshape(-1))
    lgd = dev((rng.normal(size=(B, n, K)) * 3.0).astype(np.float32).reshape(-1))
    w_in = (1.0 + 10.0 * rng.random(size=(B, n))).astype(np.float32)          # what a boundary map looks like: 1 + a exp(...)
    inl = HR.in_loss(y, K, lm)
    for keep, min_keep in ((0.3, 0), (1.0 / 3.0, 7), (1.0, 0), (0.25, 1 << 20)):
        ce0, w0, k0 = _launch(lib, B, S, K, keep, min_keep, yd, lmd, logits=lgd)
        want_w, want_k = HR.weights(ce0.cpu().numpy().reshape(B, n), inl, keep, min_keep, w_in)
        for in_place in (False, True):
            ce, w, kept = _launch(lib, B, S, K, keep, min_keep, yd, lmd, logits=lgd, w_in=dev(w_in.reshape(-1)), in_place=in_place)
            assert torch.equal(ce, ce0) and torch.equal(kept, k0)
            np.testing.assert_array_equal(kept.cpu().numpy(), want_k)
            np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32).reshape(B, n), want_w.view(np.uint32), err_msg=str((keep, min_keep, in_place)))
            if keep == 1.0 or min_keep >= n:
                got = w.cpu().numpy().reshape(B, n)
                assert (want_k == inl.sum(axis=1)).all() and (got.view(np.uint32)[inl] == w_in.view(np.uint32)[inl]).all() and not got[~inl].any()


def test_containment_and_repeatability(lib):
    """(5) guard bands around ce, weight_out and kept_out; a launch on the middle patch of three with poisoned neighbours; two launches
    give equal bits; kept_out = NULL changes nothing else"""
    B, S, K = 3, 17, 6
    n = S * S
    rng = np.random.default_rng(5)
    y, lm = _labels_and_mask(rng, B, n, K)
    lm[B - 1] = lm[0]
    lg = (rng.normal(size=(B, n, K)) * 3.0).astype(np.float32)
    yd, lmd, lgd = dev(y.reshape(-1)), dev(lm.reshape(-1)), dev(lg.reshape(-1))
    g = 64
    a = _launch(lib, B, S, K, 0.25, 5, yd, lmd, logits=lgd, guard=g)
    b = _launch(lib, B, S, K, 0.25, 5, yd, lmd, logits=lgd, guard=g)
    for t, u, m in zip(a, b, (B * n, B * n, B)):
        assert torch.equal(t, u) and (t[:g] == MARK).all() and (t[g + m:] == MARK).all() and (t[g:g + m] != MARK).all()
    c = _launch(lib, B, S, K, 0.25, 5, yd, lmd, logits=lgd, guard=g, want_kept=False)
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1]) and (c[2] == int(MARK)).all()
    # the middle patch alone, its neighbours' logits NaN and their labels and masks live: nothing of theirs is read or written
    poisoned = lg.copy()
    poisoned[0] = np.nan
    poisoned[2] = np.nan
    pd = dev(poisoned.reshape(-1))
    ce = torch.full((B * n,), MARK, dtype=torch.float32, device=DEV)
    w = torch.full((B * n,), MARK, dtype=torch.float32, device=DEV)
    kept = torch.full((B,), int(MARK), dtype=torch.int32, device=DEV)
    lib.call("drs_patch_hard_weight", pd[n * K:].data_ptr(), ce[n:].data_ptr(), yd[n:].data_ptr(), lmd[n:].data_ptr(), 1, S, K, 0.25, 5, None,
             w[n:].data_ptr(), kept[1:].data_ptr(), stream())
    torch.cuda.synchronize()
    for t, ref, m in ((ce, a[0], n), (w, a[1], n), (kept, a[2], 1)):
        assert (t[:m] == MARK).all() and (t[2 * m:] == MARK).all() and torch.equal(t[m:2 * m], ref[g + m:g + 2 * m])


# ------------------------------------------------------------------------------------------------- the step
HM = (0.25, 16)
VARIANTS = ["alone", "weights-focal", "boundary", "dice", "loss-mask"]
STEP_IDS = {"dilated_grsl": "Dilated6Pooling", "dilated_icpr_rate6_densely": "DenseDilated6"}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES, ids=[STEP_IDS[c[0]] for c in STEP_CASES])
def test_mined_step_against_fp64_autograd(net, ch, K, B, S, variant):
    """(6) the step cases and tolerances of tests/test_gpu_dice_loss.py::test_dice_step_against_fp64_autograd.  The fp64 side takes the
    weight map the step left in pixel_weight (the kernel tests hold that map), so nothing hinges on fp32-versus-fp64 rank flips at the
    threshold; the map itself must equal a direct drs_patch_hard_weight call on the step's logits."""
    from drs_amd import loops
    from drs_amd.net import DilatedNet
    WD = 0.005
    M = B * S * S
    d = DilatedNet(net, ch, K, WD, b_max=B, s_max=S, device=DEV, seed=11)
    x, y, valid = _step_inputs(ch, K, B, S, 11)
    wc, gamma, bw, dice, mask = np.ones(K, dtype=np.float32), 0.0, None, None, None
    if variant == "weights-focal":
        wc, gamma = np.asarray(WEIGHTS[K], dtype=np.float32) + 0.25, 2.0
        d.set_class_weights(wc)
        d.set_focal_gamma(gamma)
    if variant == "boundary":
        bw = BW
        d.set_boundary_weight(bw)
    if variant == "dice":
        dice = DICE
        d.set_dice(dice)
    if variant == "loss-mask":
        mask = (np.random.default_rng(5).random((B, S * S)) < 0.6).astype(np.uint8)
        mask[1] = 0                                       # a patch that is all void: n_b = 0
    d.set_hard_mining(HM)
    assert d.hard_mining == HM
    n_glob = M if mask is None else int(mask.sum())
    params = {n: d.get_variable(n).astype(np.float64) for n in d.variable_names()}
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S, mask=mask, acc_mask=valid.reshape(B, -1))
    kw = {} if mask is None else dict(use_loss_mask=True, global_pixels=n_glob)
    out = d.train_step(B, S, 0.01, apply_update=False, want_logits=True, **kw)
    torch.cuda.synchronize()
    # the map the step left = a direct call on the step's logits (and, with the boundary weight, on the map of the step's labels)
    labels = d.labels[:M].view(B, S, S)
    pw_in = None if bw is None else loops.boundary_weight_map(labels, torch.as_tensor(valid).to(DEV), *bw)[0]
    w2, ce2, kept2 = loops.hard_mining_weights(d.logits[:M * K].view(B, S, S, K), labels, HM[0], HM[1],
                                               loss_mask=None if mask is None else d.loss_mask[:M].view(B, S, S), pixel_weight=pw_in)
    assert torch.equal(w2.reshape(-1), d.pixel_weight[:M]) and torch.equal(ce2.reshape(-1), d.hard_ce[:M])
    w_step = d.pixel_weight[:M].cpu().numpy().astype(np.float64)
    n_b = np.full(B, S * S) if mask is None else mask.sum(axis=1)
    want_k = [HR.kept_count(v, *HM) for v in n_b]
    assert kept2.cpu().numpy().tolist() == want_k and ((w_step.reshape(B, -1) != 0).sum(axis=1) == want_k).all()
    if bw is not None:
        pw_ref, _ = BR.boundary_weight(y.astype(np.uint8), valid, bw[2], bw[0], 1.0 / (2.0 * bw[1] ** 2))
        scale = np.float32(S * S / want_k[0])
        keptm = w_step != 0
        assert rel_err(w_step[keptm], (scale * pw_ref.reshape(-1).astype(np.float32))[keptm]) < 1e-6
    dec = []
    for i, L in enumerate(d.plan.layers):
        z = d.z[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        mr = d.mean_rstd[i].cpu().numpy().reshape(L.cout, 2)
        dcs = {"pos": (z - mr[:, 0]) * mr[:, 1] > 0}
        if d._is_max(i):
            dcs["idx"] = d.idx[i][:M * L.cout].cpu().numpy().reshape(B, S, S, L.cout)
        dec.append(dcs)

    def total(tn):
        """the loss written with torch ops: sum w term / n with w the step's map, detached, plus the unmined Dice term"""
        for q in tn.params_list():
            q.grad = None
        logits = tn.forward(x.astype(np.float64), True)
        yy = torch.as_tensor(y.reshape(-1), dtype=torch.long)
        logp = torch.log_softmax(logits.reshape(-1, K), dim=1).gather(1, yy[:, None])[:, 0]
        l2 = sum(0.5 * (w_ ** 2).sum() for w_ in list(tn.w.values()) + list(tn.fcw.values()))
        term = torch.as_tensor(wc, dtype=torch.float64)[yy] * (-logp)
        if gamma:
            term = term * (1.0 - torch.exp(logp)) ** gamma
        ce = (torch.as_tensor(w_step) * term).sum() / n_glob
        inl = torch.ones(M, dtype=torch.float64) if mask is None else torch.as_tensor(mask.reshape(-1).astype(np.float64))
        unmined = float((inl * term).sum().detach() / n_glob)
        loss = ce + WD * l2
        if dice is not None:
            loss = loss + _torch_dice(logits if logits.shape[-1] == K else logits.permute(0, 2, 3, 1), y, K, dice, M)
        loss.backward()
        return float(loss.detach()), logits.detach().numpy(), float(ce.detach()), unmined
    forced = _ForcedTorchNet(net, ch, K, params=params, dtype=torch.float64)
    forced.dec = dec
    loss_ref, logits_ref, mined_part, unmined_part = total(forced)
    got_loss = d.loss_value(out["loss_parts"])
    print("mined step %s %s: loss %.9g forced %.9g (cross-entropy part mined %.9g, over all pixels %.9g)" % (net, variant, got_loss, loss_ref,
                                                                                                            mined_part, unmined_part))
    assert mined_part > 1.01 * unmined_part                 # the mean over the hardest quarter is larger than the mean over all
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
    # untouched: the confusion matrix counts the valid pixels, each once; an eval forward ignores the option
    cm = np.zeros((K, K), dtype=np.int64)
    ok = valid.reshape(-1) != 0
    np.add.at(cm, (y.reshape(-1)[ok], out["pred"].cpu().numpy().reshape(-1)[ok]), 1)
    np.testing.assert_array_equal(out["conf"].cpu().numpy().reshape(K, K), cm)
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S)
    _, l1 = d.forward(B, S)
    l1 = l1.clone()
    d.set_hard_mining(None)
    _, l0 = d.forward(B, S)
    assert torch.equal(l0, l1)


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES, ids=[STEP_IDS[c[0]] for c in STEP_CASES])
def test_step_engine_equals_op_level_and_repeats_bitwise(net, ch, K, B, S):
    """(7) parameters after 3 steps, hard_ce, pixel_weight: engine = op-level mirror = engine again, on top of every other loss option
    and alone"""
    from drs_amd.net import DilatedNet
    from drs_amd.engine import EngineNet
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    nets = [mk(), mk(engine=False), mk(), mk(), mk(engine=False)]
    assert isinstance(nets[0], EngineNet) and not isinstance(nets[1], EngineNet)
    for d in nets[:3]:
        d.set_class_weights(WEIGHTS[K])
        d.set_focal_gamma(2.0)
        d.set_boundary_weight(BW)
        d.set_dice(DICE)
    for d in nets:
        d.set_hard_mining(HM)
        assert d.hard_mining == HM
    off = mk()
    M = B * S * S
    for step in range(3):
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
                assert torch.equal(nets[ref].logits[:M * K], nets[i].logits[:M * K])
                assert torch.equal(nets[ref].hard_ce[:M], nets[i].hard_ce[:M])
                assert torch.equal(nets[ref].pixel_weight[:M], nets[i].pixel_weight[:M])
        assert not torch.equal(outs[3]["loss_parts"][:1], oo["loss_parts"][:1]) and not torch.equal(nets[3].grads, off.grads)
        assert not torch.equal(nets[0].grads, nets[3].grads)
        assert int((nets[3].pixel_weight[:M] != 0).sum()) == B * HR.kept_count(S * S, *HM)


def test_keep_one_or_never_set_leaves_a_training_trajectory_bitwise_unchanged():
    """(8) markers written into hard_ce and pixel_weight beforehand survive: no launch ran"""
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    a, b, c, e = mk(), mk(), mk(), mk(engine=False)
    b.set_hard_mining((1, 300))
    e.set_hard_mining(1.0)
    c.set_hard_mining(HM)
    assert type(a).__name__ == "EngineNet" and a.hard_mining is None and b.hard_mining is None and e.hard_mining is None and c.hard_mining == HM
    mark = torch.full_like(a.hard_ce, MARK)
    for d in (a, b, e):
        d.hard_ce.copy_(mark)
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
        for d in (a, b, e):
            assert torch.equal(d.hard_ce, mark) and torch.equal(d.pixel_weight, mark)          # off: no launch touches the buffers
        assert not torch.equal(a.grads, c.grads) and not torch.equal(oa["loss_parts"][:1], oc["loss_parts"][:1])


def test_dice_and_mining_share_one_inference_launch(monkeypatch):
    """(9) the op-level mirror's calls of one step (the engine equals it bit for bit, above): the inference-form classifier once"""
    from drs_amd import _lib, oplevel
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 2, 13
    x, y, valid = _step_inputs(ch, K, B, S, 3)
    real = _lib.call
    for dice, hm, bw, want in ((DICE, HM, None, ["drs_classifier_loss_pixel", "drs_patch_dice_coeffs", "drs_patch_hard_weight", "drs_classifier_loss_dice"]),
                               (None, HM, BW, ["drs_patch_boundary_weight", "drs_classifier_loss_pixel", "drs_patch_hard_weight", "drs_classifier_loss_dice"]),
                               (DICE, None, None, ["drs_classifier_loss_pixel", "drs_patch_dice_coeffs", "drs_classifier_loss_dice"]),
                               (None, None, None, ["drs_classifier_loss_dice"])):
        d = DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, engine=False)
        d.set_dice(dice)
        d.set_hard_mining(hm)
        d.set_boundary_weight(bw)
        d.feed(x.reshape(B, -1), y.reshape(B, -1), S, acc_mask=valid.reshape(B, -1))
        calls = []
        monkeypatch.setattr(oplevel._lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
        d.train_step(B, S, 0.01)
        monkeypatch.setattr(oplevel._lib, "call", real)
        torch.cuda.synchronize()
        names = [n for n, _ in calls if n in ("drs_patch_boundary_weight", "drs_classifier_loss_pixel", "drs_patch_dice_coeffs", "drs_patch_hard_weight",
                                              "drs_classifier_loss_dice")]
        assert names == want, (dice, hm, bw, names)
        inference = [a for n, a in calls if n == "drs_classifier_loss_pixel"]
        assert len(inference) == (1 if (dice or hm) else 0) and all(a[10] is None for a in inference)      # labels = NULL: logits only


def test_bad_pairs_are_rejected_by_both_nets():
    from drs_amd.net import DilatedNet
    nets = [DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV), DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV, engine=False)]
    for d in nets:
        for bad in (0, -0.5, 1.5, float("nan"), (0.5, -1), (0.5, 1 << 24), (0.5, 1.5), "0.5", (0.5, 1, 2)):
            with pytest.raises(ValueError):
                d.set_hard_mining(bad)
        assert d.hard_mining is None
        d.set_hard_mining(0.25)
        assert d.hard_mining == (0.25, 0)
        d.set_hard_mining((1, 5))
        assert d.hard_mining is None
        d.set_hard_mining((0.5, 7))
        d.set_hard_mining(None)
        assert d.hard_mining is None


# ------------------------------------------------------------------------------------------------- two ranks
# (10) the spawn pattern of tests/test_gpu_dice_loss.py::test_two_rank_step_follows_the_single_rank_step on that test's inputs.  The
# per-patch selection is what this test exists for: each rank ranks its own patches only, so the ranks' maps side by side must BE the
# single rank's map, and the loss must agree to 1e-6 ABSOLUTE as in tests/test_gpu_dp.py::test_two_rank_step_equals_single_rank.
# Gradients and parameters: that test's bounds (2e-3, 1e-4) are what the ReLU signs and pool winners that flip on last-bit
# differences of the all-reduced batch statistics cost at UNIT pixel weight.  A flipped decision changes the gradient by
# the weight of the pixels behind it, and a kept pixel carries n_b / k_b times the unit weight under an unchanged normaliser, so the
# bounds here are those bounds times n_b / k_b (3.97 at keep = 0.25, 441 pixels) -- the worst case, the gradient's own maximum not
# growing.  Measured with equal maps and a loss difference of 2e-7: gradients 4.3e-3, parameters 1.4e-4.
DP = ("dilated8_grsl", 5, 6, 4, 21)
DP_HM = (0.25, 0)


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
    loops.setup_hard_mining(d, DP_HM, comm, lambda *a: None)          # what the loops do: one agree on the pair
    d.feed(x[sl], y[sl], S)
    res = d.train_step(B // world, S, 0.01)
    torch.cuda.synchronize()
    np.savez(out + "_rank%d.npz" % rank, grads=d.grads.cpu().numpy(), params=d.params.cpu().numpy(), bn=d.bn.cpu().numpy(),
             loss=d.loss_value(res["loss_parts"]), conf=res["conf"].cpu().numpy(), hm=np.asarray(d.hard_mining),
             weight=d.pixel_weight[:(B // world) * S * S].cpu().numpy())
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_step_follows_the_single_rank_step(tmp_path):
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    out = str(tmp_path) + "/dp"
    mp.spawn(_dp_worker, args=(2, 31800 + os.getpid() % 1000, out), nprocs=2, join=True)
    x, y = _dp_inputs()
    losses = {}
    for hm in (None, DP_HM):                # (the step without mining too, to show below that it mattered)
        d = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=3)
        d.set_hard_mining(hm)
        d.feed(x, y, S)
        res = d.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        losses[hm] = d.loss_value(res["loss_parts"])
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    assert tuple(r0["hm"]) == tuple(r1["hm"]) == DP_HM
    loss = losses[DP_HM]
    print("two ranks: loss %.9g (rank 0 %.9g), without mining %.9g" % (loss, float(r0["loss"]), losses[None]))
    assert abs(loss - losses[None]) > 1e-2 * losses[None]
    # the ranks' maps, side by side, are the whole batch's map: the same pixels kept at the same weight
    whole = d.pixel_weight[:B * S * S].cpu().numpy()
    both = np.concatenate([r0["weight"], r1["weight"]])
    print("two ranks: %d of %d pixels differ between the ranks' maps and the single rank's" % (int((both != whole).sum()), whole.size))
    np.testing.assert_array_equal(both, whole)

    def rel(a, b):
        return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))
    print("two ranks: grads %.3g params %.3g bn %.3g" % (rel(r0["grads"], d.grads.cpu().numpy()), rel(r0["params"], d.params.cpu().numpy()),
                                                        rel(r0["bn"], d.bn.cpu().numpy())))
    scale = S * S / HR.kept_count(S * S, *DP_HM)
    assert abs(float(r0["loss"]) - loss) < 1e-6
    assert rel(r0["grads"], d.grads.cpu().numpy()) < 2e-3 * scale
    assert rel(r0["params"], d.params.cpu().numpy()) < 1e-4 * scale
    assert rel(r0["bn"], d.bn.cpu().numpy()) < 1e-6
    np.testing.assert_array_equal(r0["conf"], res["conf"].cpu().numpy())
    np.testing.assert_array_equal(r0["params"], r1["params"])


# ------------------------------------------------------------------------------------------------- loop and command lines
def test_train_loop_prints_the_mined_loss_and_keeps_the_pair(tmp_path, capsys, monkeypatch):
    """(11) the printed loss is that of the mined loss: the mean over the step's weight map times the fp64 cross-entropy of its logits"""
    from drs_amd import loops, sampling as SP
    from drs_amd.engine import EngineNet
    from drs_amd.synthetic import make_tile
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
                     out["loss_parts"].cpu().numpy().copy(), self.pixel_weight[:M].cpu().numpy().astype(np.float64).reshape(B, S * S)))
        return out
    monkeypatch.setattr(EngineNet, "train_step", recording)
    out = str(tmp_path) + "/"
    net = loops.train(data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 4, WD, mean, std, "loss", "single_fixed",
                      [13], None, None, None, None, 20, out, 1, "dilated_grsl", "vaihingen", "none", device=DEV,
                      val_cache_dir=str(tmp_path), hard_mining=(0.25, 16))
    text = capsys.readouterr().out
    assert "Hard mining: keep 0.25 min_keep 16" in text and "Focal loss" not in text and "Dice term" not in text
    assert net.hard_mining == (0.25, 16) and net.focal_gamma == 0.0 and net.dice is None
    printed = [float(v) for v in re.findall(r"Training Minibatch: Loss= ([0-9.eE+-]+)", text)]
    assert len(printed) == len(seen) == 4
    for got, (lg, lab, parts, w) in zip(printed, seen):
        ce = HR.cross_entropy(lg, lab.astype(np.int64))
        assert ((w != 0).sum(axis=1) == HR.kept_count(169, 0.25, 16)).all() and (w[w != 0] == np.float32(169 / 43)).all()
        want = float((w * ce).mean()) + WD * float(parts[1])
        plain = float(ce.mean()) + WD * float(parts[1])
        print("loop loss printed %.6f mined %.6f over all pixels %.6f" % (got, want, plain))
        assert abs(got - want) < 1e-4 * min(1.0, abs(want)) and want > 1.05 * plain
    assert os.path.isfile(out + "hard_mining_step_4.npy") and not os.path.exists(out + "dice_step_4.npy")
    assert np.load(out + "hard_mining_step_4.npy").tolist() == [0.25, 16.0]
    # a resumed run trains the same loss and says so; a pair given on a resumed run replaces the restored one, and the log says that too
    args = (data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 5, WD, mean, std, "loss", "single_fixed", [13], None, None, None,
            None, 20, out, 1, "dilated_grsl", "vaihingen", out + "model-4")
    net2 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path))
    text = capsys.readouterr().out
    assert "Hard mining (restored from " + out + "hard_mining_step_4.npy): keep 0.25 min_keep 16" in text and net2.hard_mining == (0.25, 16)
    net3 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path), hard_mining=0.5, focal_gamma=2.0)
    text = capsys.readouterr().out
    assert "Hard mining: keep 0.5 min_keep 0" in text
    assert "replacing the pair restored from the checkpoint, keep 0.25 min_keep 16" in text
    assert "Focal loss: gamma 2" in text and net3.hard_mining == (0.5, 0) and net3.focal_gamma == 2.0


def test_the_three_command_lines_take_the_option(tmp_path, monkeypatch, capsys):
    """one smoke per flavour, at the shapes of tests/test_gpu_loops.py's command-line tests"""
    from drs_amd import cli
    monkeypatch.chdir(tmp_path)           # the reference keeps its .npy caches in the cwd
    out = str(tmp_path) + "/out_"
    random.seed(0)
    np.random.seed(0)
    net = cli.main(["isprs_dilated_random.py", "--hard-mining=0.25,16", "synthetic:70x80x5/vaihingen/", out, "none", "a,b", "c", "0.01", "0.005",
                    "4", "2", "25", "10", "dilated8_grsl", "multi_fixed", "9,13", "acc", "training"], device=DEV)
    assert net.global_step == 2 and net.hard_mining == (0.25, 16) and os.path.isfile(out + "hard_mining_step_2.npy")
    net = cli.main_coffee(["coffee_dilated_random.py", "synthetic:2x60x60x3/", "synthetic:1x60x60x3/", out, "none", "0.01", "0.001", "6",
                           "2", "25", "10", "dilated_icpr_rate6_small", "multi_fixed", "9,13", "loss", "--hard-mining=0.5"], device=DEV)
    assert net.plan.K == 2 and net.global_step == 2 and net.hard_mining == (0.5, 0)
    net = cli.main_contest(["contest_dilated_random.py", "synthetic:80x70x3/", out, "none", "0.01", "0.001", "4", "2", "25", "10",
                            "dilated_grsl", "multi_fixed", "9,13", "acc", "train", "--hard-mining=0.3,8", "--dice-weight=1"], device=DEV)
    assert net.plan.K == 7 and net.global_step == 2 and net.hard_mining == (0.3, 8) and net.dice == (1.0, 0.5, 0.5, 1.0)
