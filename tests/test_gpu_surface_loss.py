"""-m gpu: the boundary (surface) loss of the training loss from the kernel up: the signed squared distances of
drs_patch_surface_loss bit for bit against the numpy statement (tests/surface_loss_ref.py, itself held by
tests/test_surface_loss_plan.py against scipy and a brute-force minimum), the map and the patches' terms against fp64, accumulate and
the Dice fold, the three forms of the fused classifier with the map against the fp64 closed form, a whole training step against fp64
autograd, engine = op level, lam = 0, two ranks, the training loop and the three command lines.

Tolerances are the project's existing ones: single ops 1e-5 relative to the tensor's maximum and 1e-6 for a loss, whole nets 1e-4
(logits 1e-3), two ranks as tests/test_gpu_dp.py.  A patch's term sum g_c P_c is signed and cancels (phi is positive outside a class
and negative inside), so its 1e-6 is relative to sum |g_c P_c| of the patch, what the fp32 probabilities' errors scale with."""
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
import surface_loss_ref as SR   # noqa: E402
from gpu_util import DEV, dev, rel_err, stream   # noqa: E402
from test_gpu_class_weights import WEIGHTS, _feed_step, _ForcedTorchNet   # noqa: E402  (helpers only)
from test_gpu_focal_loss import FORMS, _check_form, _moderate   # noqa: E402  (helpers only: the form table, its shared inputs)
from test_gpu_dice_loss import _Dc, _coefficients_of, _mode, _step_inputs, _torch_dice, MODES, STEP_CASES, DICE, BW   # noqa: E402  (helpers only)
from test_gpu_lovasz import _Rg, _torch_lovasz, HM, LOV, MARK   # noqa: E402  (helpers only)


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# ------------------------------------------------------------------------------------------------- the pre-pass kernel
# (1, 128, 2) and (1, 129, 2): the largest side whose planes stay in LDS and the smallest whose planes go through scratch
SHAPES = [(1, 1, 2), (2, 13, 3), (3, 16, 6), (2, 37, 8), (1, 64, 6), (1, 128, 2), (1, 129, 2)]
LAMS = {1: (1.0, 0.0), 13: (2.5, 3.0), 16: (1.5, 0.0), 37: (64.0, 32768.0), 64: (0.75, 10.0), 128: (1.5, 0.0), 129: (1.5, 50.0)}
G = 64          # guard words around every output


def _blobs(rng, B, S, K):
    c = max(1, S // 4)
    coarse = rng.integers(0, K, size=(B, (S + c - 1) // c, (S + c - 1) // c))
    return np.repeat(np.repeat(coarse, c, axis=1), c, axis=2)[:, :S, :S].astype(np.uint8)


def _inputs(B, S, K, seed):
    """name -> (logits float32 [B, S, S, K], labels uint8 [B, S, S], loss mask uint8 or None, valid uint8 or None)"""
    rng = np.random.default_rng(seed)
    lg = (rng.normal(size=(B, S, S, K)) * 3.0).astype(np.float32)
    blobs = _blobs(rng, B, S, K)
    speckle = rng.integers(0, K, size=(B, S, S)).astype(np.uint8)
    lone = np.zeros((B, S, S), dtype=np.uint8)
    lone[:, 0, 0] = K - 1                               # one pixel in a corner: every other pixel scans to the far end, no early exit
    lone[0, 0, 0], lone[0, S - 1, S - 1] = 0, K - 1     # ... and in the opposite corner in patch 0
    sx = np.broadcast_to(((np.arange(S) // 3) % K).astype(np.uint8)[None, None, :], (B, S, S)).copy()
    sy = np.broadcast_to(((np.arange(S) // 2) % K).astype(np.uint8)[None, :, None], (B, S, S)).copy()
    y = blobs.copy()
    out = rng.random(size=y.shape) < 0.05
    y[out] = rng.choice([K, 255], size=int(out.sum())).astype(np.uint8)
    y[0][y[0] == K - 1] = 0                             # class K - 1 absent from patch 0
    lm = (rng.random(size=y.shape) < 0.8).astype(np.uint8)
    va = (rng.random(size=y.shape) < 0.8).astype(np.uint8)
    if B > 1:
        va[B - 1] = 0                                   # a last patch with nothing counted
    return {"blobs": (lg, blobs, None, None), "speckle": (lg, speckle, None, None), "lone-pixel": (lg, lone, None, None),
            "stripes-x": (lg, sx, None, None), "stripes-y": (lg, sy, None, None), "mixed": (lg, y, lm, va),
            "single-class": (lg, np.full((B, S, S), K - 1, dtype=np.uint8), None, None),
            "nothing-counted": (lg, blobs, np.zeros_like(lm), None)}


class _Pre(object):
    """one call of drs_patch_surface_loss with guard words around every output and around scratch"""

    def __init__(self, lib, lg, y, lm, va, B, S, K, lam, clip, dice=None, accumulate=0, want_phi2=True, scratch_fill=0, grad_init=None):
        M = B * S * S
        self.lgd = None if lg is None else dev(lg.reshape(-1))
        self.yd, self.lmd, self.vad = dev(y.reshape(-1)), None if lm is None else dev(lm.reshape(-1)), None if va is None else dev(va.reshape(-1))
        self.phi2 = torch.full((M * K + 2 * G,), 12345, dtype=torch.int32, device=DEV) if want_phi2 else None
        self.grad = torch.full((M * K + 2 * G,), MARK, dtype=torch.float32, device=DEV)
        if grad_init is not None:
            self.grad[G:G + M * K] = dev(grad_init.reshape(-1).astype(np.float32))
        self.pl = torch.full((B + 2 * G,), MARK, dtype=torch.float64, device=DEV)
        nbytes = lib.query("drs_surface_loss_scratch_bytes", B, S, K)
        assert nbytes > 0 and nbytes % 16 == 0
        self.scratch = torch.full((nbytes + 2 * G,), scratch_fill, dtype=torch.uint8, device=DEV)
        self.dice = None if dice is None else dev(dice.reshape(-1).astype(np.float32))
        lib.call("drs_patch_surface_loss", None if self.lgd is None else self.lgd.data_ptr(), self.yd.data_ptr(),
                 None if self.lmd is None else self.lmd.data_ptr(), None if self.vad is None else self.vad.data_ptr(), B, S, K, lam, clip,
                 None if self.dice is None else self.dice.data_ptr(), accumulate, None if self.phi2 is None else self.phi2[G:].data_ptr(),
                 self.grad[G:].data_ptr(), self.pl[G:].data_ptr(), self.scratch[G:].data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        self.shape, self.nbytes, self.fill = (B, S, K), nbytes, scratch_fill

    def host(self):
        B, S, K = self.shape
        M = B * S * S
        p2 = None if self.phi2 is None else self.phi2[G:G + M * K].cpu().numpy().astype(np.int64).reshape(B, S, S, K)
        return p2, self.grad[G:G + M * K].cpu().numpy().reshape(B, S, S, K), self.pl[G:G + B].cpu().numpy()

    def guards_ok(self):
        B, S, K = self.shape
        M = B * S * S
        ok = bool((self.grad[:G] == MARK).all() and (self.grad[G + M * K:] == MARK).all() and (self.pl[:G] == MARK).all() and
                  (self.pl[G + B:] == MARK).all())
        ok = ok and bool((self.scratch[:G] == self.fill).all() and (self.scratch[G + self.nbytes:] == self.fill).all())
        if self.phi2 is not None:
            ok = ok and bool((self.phi2[:G] == 12345).all() and (self.phi2[G + M * K:] == 12345).all())
        return ok


@pytest.mark.parametrize("B,S,K", SHAPES, ids=["%dx%dx%d-K%d" % (b, s, s, k) for b, s, k in SHAPES])
def test_prepass_against_the_statement(lib, B, S, K):
    lam, clip = LAMS[S]
    sums = (B * K * 8 + 15) // 16 * 16
    nbytes = lib.query("drs_surface_loss_scratch_bytes", B, S, K)
    assert (nbytes == sums) == (S <= 128) and (nbytes >= sums + B * K * 4 * S * S) == (S > 128)          # which storage form this shape takes
    for name, (lg, y, lm, va) in _inputs(B, S, K, seed=100 * S + K).items():
        r = _Pre(lib, lg, y, lm, va, B, S, K, lam, clip)
        phi2, grad, pl = r.host()
        assert r.guards_ok(), name
        ref = SR.surface_loss(lg, y, K, lam, clip, loss_mask=lm, valid=va)
        cnt = ref["counted"]
        if name == "mixed" and S > 1:
            assert (y >= K).any() and not ref["phi2"][0, :, :, K - 1].any() and (B == 1 or not cnt[B - 1].any())
            assert not cnt.all() and (ref["phi2"][0].any() or K == 2)       # (K = 2: patch 0 is left with one class, no contour)
        if name in ("nothing-counted", "single-class") or S == 1:
            assert not ref["phi2"].any()
        elif name != "mixed":
            assert ref["phi2"].any() and cnt.all()
        if name == "lone-pixel" and S > 1:
            assert ref["phi2"][0, 0, 0, K - 1] == 2 * (S - 1) ** 2                       # the far diagonal
        # the signed squared distances: exactly the statement's
        np.testing.assert_array_equal(phi2, ref["phi2"], err_msg=name)
        # the map: within one fp32 rounding of the fp64 value, exact +0 where phi is 0 or the pixel is not counted
        g = ref["g"]
        assert (np.abs(grad.astype(np.float64) - g) <= 2.0 ** -23 * np.abs(g)).all(), name
        zero = (g == 0) | ~cnt[..., None]
        assert not grad[zero].any() and not np.signbit(grad[zero]).any(), name
        if clip:
            assert np.abs(grad).max() <= np.float32(lam * clip)
        # the patches' terms: 1e-6 of the fp64 statement, relative to sum |g_c P_c| (the term is signed and cancels)
        e_pl = np.abs(pl - ref["patch_loss"])
        print("surface pre-pass %dx%dx%d K%d %s: patch_loss error %.3g of sum |g P| (the sum itself %.3g of it)" % (
            B, S, S, K, name, float((e_pl / np.maximum(ref["abs_sum"], 1e-300)).max()),
            float((np.abs(ref["patch_loss"]) / np.maximum(ref["abs_sum"], 1e-300)).max())))
        assert (e_pl <= 1e-6 * ref["abs_sum"]).all(), (name, e_pl, ref["abs_sum"])
        empty = ~cnt.reshape(B, -1).any(axis=1)
        assert not pl[empty].any() and not grad[empty].any()
        # phi2_out = NULL gives the same map and terms, a second run the same bits, scratch full of 0xFF bytes the same bits as zeroed scratch
        r2 = _Pre(lib, lg, y, lm, va, B, S, K, lam, clip, want_phi2=False)
        r3 = _Pre(lib, lg, y, lm, va, B, S, K, lam, clip, scratch_fill=0xFF)
        r4 = _Pre(lib, lg, y, lm, va, B, S, K, lam, clip)
        for other in (r2, r3, r4):
            assert torch.equal(other.grad, r.grad) and torch.equal(other.pl, r.pl) and other.guards_ok(), name
        assert torch.equal(r3.phi2, r.phi2) and torch.equal(r4.phi2, r.phi2)
        # logits = NULL: the same map and distances, the terms written as 0
        r5 = _Pre(lib, None, y, lm, va, B, S, K, lam, clip)
        assert torch.equal(r5.grad, r.grad) and torch.equal(r5.phi2, r.phi2) and r5.guards_ok() and not r5.pl[G:G + B].any()


def test_accumulate_adds_with_one_fp32_add_and_leaves_uncounted_entries_alone(lib):
    B, S, K = 3, 16, 6
    lg, y, lm, va = _inputs(B, S, K, seed=9)["mixed"]
    rng = np.random.default_rng(9)
    marked = rng.normal(size=(B, S, S, K)).astype(np.float32)
    a = _Pre(lib, lg, y, lm, va, B, S, K, 1.5, 4.0)
    b = _Pre(lib, lg, y, lm, va, B, S, K, 1.5, 4.0, accumulate=1, grad_init=marked)
    p2a, ga, pla = a.host()
    p2b, gb, plb = b.host()
    cnt = SR.counted(y, K, lm, va)
    want = np.where(cnt[..., None], marked + ga, marked)
    np.testing.assert_array_equal(gb, want)
    np.testing.assert_array_equal(p2a, p2b)
    np.testing.assert_array_equal(pla, plb)
    assert b.guards_ok() and ga[cnt].any() and not cnt.all() and (gb[~cnt] == marked[~cnt]).all()


def test_prepass_folds_the_dice_coefficients_in_with_one_add(lib):
    B, S, K = 3, 16, 6
    lg, y, lm, va = _inputs(B, S, K, seed=9)["mixed"]
    rng = np.random.default_rng(9)
    coef = np.stack([-rng.random((B, K)), rng.random((B, K))], axis=2).astype(np.float32)
    a, b = _Pre(lib, lg, y, lm, va, B, S, K, 1.5, 0.0), _Pre(lib, lg, y, lm, va, B, S, K, 1.5, 0.0, dice=coef)
    p2a, ga, pla = a.host()
    p2b, gb, plb = b.host()
    inl = LR.in_loss(y, K, lm)                                   # in the loss whatever `valid` says: where the Dice term lives
    onehot = y[..., None] == np.arange(K)
    want = ga + np.where(onehot, coef[:, None, None, :, 0], coef[:, None, None, :, 1])
    want[~inl] = 0
    np.testing.assert_array_equal(gb, want)
    np.testing.assert_array_equal(p2a, p2b)
    np.testing.assert_array_equal(pla, plb)
    cnt = SR.counted(y, K, lm, va)
    assert (inl & ~cnt).any() and gb[inl & ~cnt].all()               # in the loss but not valid: the Dice part alone
    assert gb[0][inl[0]][:, K - 1].all() and not p2b[0, :, :, K - 1].any()        # an absent class still carries its Dice part
    # both at once is refused, and nothing is written
    from drs_amd import _lib as L
    grad = torch.full((B * S * S * K,), MARK, dtype=torch.float32, device=DEV)
    rc = L.load().drs_patch_surface_loss(None, a.yd.data_ptr(), None, None, B, S, K, 1.5, 0.0, b.dice.data_ptr(), 1, None, grad.data_ptr(),
                                          a.pl[G:].data_ptr(), a.scratch[G:].data_ptr(), a.nbytes, None)
    torch.cuda.synchronize()
    assert rc == 1 and (grad == MARK).all()


def test_loops_surface_loss_grad_returns_the_direct_calls_bits(lib):
    from drs_amd import loops
    B, S, K = 2, 13, 3
    lg, y, lm, va = _inputs(B, S, K, seed=4)["mixed"]
    grad, phi2, pl = loops.surface_loss_grad(lg, y, 2.5, 3.0, loss_mask=lm, valid=va)
    r = _Pre(lib, lg, y, lm, va, B, S, K, 2.5, 3.0)
    p2, g2, pl2 = r.host()
    np.testing.assert_array_equal(grad.cpu().numpy(), g2)
    np.testing.assert_array_equal(phi2.cpu().numpy(), p2)
    np.testing.assert_array_equal(pl.cpu().numpy(), pl2)
    assert phi2.dtype == torch.int64 and tuple(grad.shape) == (B, S, S, K)
    grad0, _, _ = loops.surface_loss_grad(torch.from_numpy(lg).to(DEV), torch.from_numpy(y).to(DEV), 2.5)
    np.testing.assert_array_equal(grad0.cpu().numpy(), _Pre(lib, lg, y, None, None, B, S, K, 2.5, 0.0).host()[1])
    with pytest.raises(ValueError):
        loops.surface_loss_grad(lg, y, 2.5, 0.5)


# ------------------------------------------------------------------------------------------------- the classifier with the map
LAM, CLIP = 1.5, 6.0
LMODES = {"alone": MODES["dice-alone"], "on-weights-focal-map": MODES["on-weights-focal-map"]}
LCASES = [(f, m) for f in FORMS for m in LMODES]
_SURF = {}


def _surface_of(lib, d, form):
    """the step's pre-pass on the form's inputs (the map from the logits of the plain launch, valid = the accuracy mask) and the fp64
    statement on the form's fp64 logits: computed once per form, shared by the modes, left unchanged"""
    if form not in _SURF:
        C, K, B, S, P = FORMS[form]
        M = B * S * S
        grad = torch.zeros(M * K, dtype=torch.float32, device=DEV)
        pl = torch.zeros(B, dtype=torch.float64, device=DEV)
        nbytes = lib.query("drs_surface_loss_scratch_bytes", B, S, K)
        scratch = torch.zeros(nbytes // 8, dtype=torch.float64, device=DEV)
        lib.call("drs_patch_surface_loss", d["plain"].logits.data_ptr(), d["yd"].data_ptr(), d["lmd"].data_ptr(), d["amd"].data_ptr(), B, S, K,
                 LAM, CLIP, None, 0, None, grad.data_ptr(), pl.data_ptr(), scratch.data_ptr(), nbytes, stream())
        torch.cuda.synchronize()
        y = d["yd"].cpu().numpy().reshape(B, S, S)
        lm, am = d["lmd"].cpu().numpy().reshape(B, S, S), d["amd"].cpu().numpy().reshape(B, S, S)
        ref = SR.surface_loss(d["lg_ref"].reshape(B, S, S, K), y, K, LAM, CLIP, loss_mask=lm, valid=am, inv_n=1.0 / d["n"])
        _SURF[form] = (grad, pl, ref)
    return _SURF[form]


@pytest.mark.parametrize("form,mode", LCASES, ids=["%s-%s" % c for c in LCASES])
def test_region_classifier_with_the_surface_map_against_fp64_numpy(lib, form, mode):
    """the structure and tolerances of tests/test_gpu_lovasz.py::test_region_classifier_against_fp64_numpy"""
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
    region, pl, sv = _surface_of(lib, d, form)
    assert sv["counted"].any() and not sv["counted"].reshape(-1)[~inl].any() and (inl & ~sv["counted"].reshape(-1)).any()
    np.testing.assert_array_equal(region.cpu().numpy().reshape(M, K), sv["g32"].reshape(M, K))       # the same distances: the same fp32 map
    gl = gl_ce + sv["grad"].reshape(M, K)
    w64, f64 = d["w64"], d["f64"]
    gf_ce, gf = gl_ce @ w64.T, gl @ w64.T
    share = float(np.linalg.norm(gf - gf_ce) / np.linalg.norm(gf_ce))
    assert share > 1e-2, share                          # the term changes gfeat by more than 1 % in norm
    r = _Rg(lib, d, form, wc, gamma, None if pw is None else dev(pw), region)
    plain = d["plain"]
    assert torch.equal(r.logits, plain.logits) and torch.equal(r.pred, plain.pred) and torch.equal(r.conf, plain.conf)
    abs_loss = float(sv["abs_sum"].sum() / d["n"])
    figures = dict(ce_loss=abs(r.ls.item() / d["n"] - ce_loss) / abs(ce_loss),
                   loss=abs((r.ls.item() + pl.sum().item()) / d["n"] - (ce_loss + sv["loss"])) / (abs(ce_loss) + abs_loss),
                   surface_loss=abs(pl.sum().item() / d["n"] - sv["loss"]) / abs_loss,
                   gfeat=rel_err(r.gfeat.cpu().numpy().reshape(M, C), gf), dw=rel_err(r.dw.cpu().numpy().reshape(C, K), f64.T @ gl),
                   db=rel_err(r.db.cpu().numpy(), gl.sum(axis=0)), share=share)
    print("region classifier with the surface map %s %s: %s" % (form, mode, figures))
    assert not r.gfeat.view(M, C)[torch.from_numpy(~inl).to(DEV)].any()          # not in the loss: exact zeros
    assert np.isfinite(r.gfeat.cpu().numpy()).all()
    assert figures["ce_loss"] < 1e-6 and figures["loss"] < 1e-6 and figures["surface_loss"] < 1e-6
    assert figures["gfeat"] < 1e-5 and figures["dw"] < 1e-5 and figures["db"] < 1e-5


# ------------------------------------------------------------------------------------------------- the step
SURF = (0.5, 6.0)


def _torch_surface(logits, g, n_glob):
    """L_surf written with torch ops: softmax times the constant map (0 where a pixel is not counted), summed, over n_glob"""
    K = g.shape[-1]
    p = torch.softmax(logits.reshape(-1, K), dim=1)
    return (p * torch.as_tensor(g.reshape(-1, K).astype(np.float64))).sum() / n_glob


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES, ids=["Dilated6Pooling", "DenseDilated6"])
def test_surface_step_against_fp64_autograd(net, ch, K, B, S):
    """on top of class weights, the focal factor, the boundary weight, the Dice term, hard mining and the Lovasz term.
    Decision-aligned as the project's step tests are: ReLU signs, pool winners and the mined weight map from the device, and the order
    of every (patch, class) of the Lovasz term from the device's fp32 logits; the distance maps are the numpy statement's"""
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
    d.set_surface_loss(SURF)
    assert d.surface_loss == SURF and d.lovasz == LOV and d.dice == DICE and d.hard_mining == HM
    params = {n: d.get_variable(n).astype(np.float64) for n in d.variable_names()}
    d.feed(x.reshape(B, -1), y.reshape(B, -1), S, acc_mask=valid.reshape(B, -1))
    out = d.train_step(B, S, 0.01, apply_update=False, want_logits=True)
    torch.cuda.synchronize()
    # the map the step left = direct calls on the step's logits: the Lovasz map with the step's Dice coefficients, the surface map added
    lg4, lab3 = d.logits[:M * K].view(B, S, S, K), d.labels[:M].view(B, S, S)
    g2, rank, err2, pl2 = loops.lovasz_grad(lg4, lab3, LOV, dice_coef=d.dice_coef[:B * K * 2].view(B, K, 2))
    gs, phi2, pls = loops.surface_loss_grad(lg4, lab3, SURF[0], SURF[1], valid=d.acc_mask[:M].view(B, S, S))
    cnt = torch.from_numpy(valid.reshape(B, S, S) != 0).to(DEV)
    assert torch.equal(torch.where(cnt[..., None], g2 + gs, g2).reshape(-1), d.region_grad[:M * K])
    assert torch.equal(pl2, d.lovasz_loss[:B]) and torch.equal(pls, d.surface_loss_terms[:B])
    sv = SR.surface_loss(lg4.cpu().numpy().astype(np.float64), y, K, SURF[0], SURF[1], valid=valid, inv_n=1.0 / M)
    np.testing.assert_array_equal(phi2.cpu().numpy(), sv["phi2"])
    np.testing.assert_array_equal(gs.cpu().numpy(), sv["g32"])
    assert not valid.all() and sv["phi2"].any()                                                   # fill pixels are not counted
    print("surface step %s: |phi| up to %.3g pixels, clip %g" % (net, float(np.abs(sv["phi"]).max()), SURF[1]))
    rank = rank.cpu().numpy().reshape(B, S * S, K)
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
        surf = _torch_surface(lg_nhwc, sv["g32"], M)
        loss = ce + _torch_dice(lg_nhwc, y, K, DICE, M) + _torch_lovasz(lg_nhwc, y, K, LOV, M, rank) + surf + WD * l2
        loss.backward()
        return float(loss.detach()), logits.detach().numpy(), float(surf.detach())
    forced = _ForcedTorchNet(net, ch, K, params=params, dtype=torch.float64)
    forced.dec = dec
    loss_ref, logits_ref, surf_part = total(forced)
    got_loss = d.loss_value(out["loss_parts"])
    print("surface step %s: loss %.9g forced %.9g (the surface term %.9g)" % (net, got_loss, loss_ref, surf_part))
    # the term matters: it is signed and cancels (with K = 2, phi_0 = 1 - phi_1 up to the contour's pixel, and P_0 + P_1 = 1), so
    # its weight in the step is sum |g_c P_c| over the global pixels, not the sum itself
    assert float(sv["abs_sum"].sum()) / M > 1e-2 * abs(loss_ref)
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
    d.set_surface_loss(None)
    _, l0 = d.forward(B, S)
    assert torch.equal(l0, l1)


def test_surface_step_with_a_loss_mask_gives_a_void_patch_exactly_zero():
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
    for s in (None, SURF):
        d.set_surface_loss(s)
        d.feed(x.reshape(B, -1), y.reshape(B, -1), S, mask=mask)
        out = d.train_step(B, S, 0.01, use_loss_mask=True, global_pixels=n, apply_update=False, want_logits=True)
        torch.cuda.synchronize()
        losses[s] = float(out["loss_parts"][0].item())
    lg = d.logits[:B * S * S * K].cpu().numpy().astype(np.float64).reshape(B, S, S, K)
    ref = SR.surface_loss(lg, y, K, SURF[0], SURF[1], loss_mask=mask.reshape(B, S, S), inv_n=1.0 / n)
    scale = float(ref["abs_sum"].sum() / n)
    assert not ref["counted"][1].any() and ref["patch_loss"][1] == 0 and scale > 1e-2 * losses[None]
    print("surface step with a loss mask: %.9g = %.9g + %.9g (sum |g P| %.9g)" % (losses[SURF], losses[None], ref["loss"], scale))
    assert abs(losses[SURF] - losses[None] - ref["loss"]) < 1e-6 * (losses[None] + scale)
    assert not d.region_grad[:B * S * S * K].view(B, S * S, K)[1].any() and d.surface_loss_terms[1].item() == 0


@pytest.mark.parametrize("net,ch,K,B,S", STEP_CASES)
def test_step_engine_equals_op_level_and_repeats_bitwise(net, ch, K, B, S):
    from drs_amd.net import DilatedNet
    from drs_amd.engine import EngineNet
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    nets = [mk(), mk(engine=False), mk(), mk(), mk(engine=False)]
    assert isinstance(nets[0], EngineNet) and not isinstance(nets[1], EngineNet)
    for d in nets[:3]:                       # stacked on class weights, the focal term, the boundary weight, the Dice term, mining and Lovasz ...
        d.set_class_weights(WEIGHTS[K])
        d.set_focal_gamma(2.0)
        d.set_boundary_weight(BW)
        d.set_dice(DICE)
        d.set_hard_mining(HM)
        d.set_lovasz(LOV)
    for d in nets:                           # ... and alone
        d.set_surface_loss(SURF)
        assert d.surface_loss == SURF
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
                assert torch.equal(nets[ref].region_grad[:n], nets[i].region_grad[:n])
                assert torch.equal(nets[ref].surface_loss_terms[:B], nets[i].surface_loss_terms[:B])
        assert not torch.equal(outs[3]["loss_parts"][:1], oo["loss_parts"][:1]) and not torch.equal(nets[3].grads, off.grads)
        assert not torch.equal(nets[0].grads, nets[3].grads)


def test_lambda_zero_or_never_set_leaves_a_training_trajectory_bitwise_unchanged():
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    a, b, c, e = mk(), mk(), mk(), mk(engine=False)
    b.set_surface_loss((0, 8))
    e.set_surface_loss(0.0)
    c.set_surface_loss(SURF)
    assert type(a).__name__ == "EngineNet" and a.surface_loss is None and b.surface_loss is None and e.surface_loss is None and c.surface_loss == SURF
    names = ("surface_loss_terms", "surface_scratch", "region_grad")
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


def test_surface_loss_without_lovasz_takes_the_write_path(lib):
    """Lovasz off: accumulate = 0, the Dice coefficients folded in when that term is on, else a plain write; the engine's step equals the
    op-level mirror, whose calls are recorded"""
    from drs_amd import loops
    from drs_amd.net import DilatedNet
    net, ch, K, B, S = "dilated_grsl", 5, 6, 3, 19
    M = B * S * S
    mk = lambda **kw: DilatedNet(net, ch, K, 0.005, b_max=B, s_max=S, device=DEV, seed=7, **kw)   # noqa: E731
    x, y, valid = _step_inputs(ch, K, B, S, 40)
    for dice, lov in ((None, None), (DICE, None), (DICE, LOV)):
        a, e = mk(), mk(engine=False)
        calls = []
        real = lib.call
        for d in (a, e):
            d.set_dice(dice)
            d.set_lovasz(lov)
            d.set_surface_loss(SURF)
            d.region_grad.fill_(MARK)
        oa = _feed_step(a, x.reshape(B, -1), y.reshape(B, -1), S, want_logits=True)
        lib.call = lambda name, *args: (calls.append((name, args)), real(name, *args))[1]
        try:
            oe = _feed_step(e, x.reshape(B, -1), y.reshape(B, -1), S, want_logits=True)
        finally:
            lib.call = real
        torch.cuda.synchronize()
        names = [c[0] for c in calls]
        assert names.count("drs_patch_surface_loss") == 1 and names.count("drs_classifier_loss_region") == 1 and "drs_classifier_loss_dice" not in names
        assert names.count("drs_classifier_loss_pixel") == 1                        # one inference-form launch for all pre-passes
        assert ("drs_patch_lovasz_grad" in names) == (lov is not None) and ("drs_patch_dice_coeffs" in names) == (dice is not None)
        args = [c[1] for c in calls if c[0] == "drs_patch_surface_loss"][0]
        assert args[10] == (0 if lov is None else 1) and (args[9] is not None) == (dice is not None and lov is None)
        assert names.index("drs_patch_surface_loss") < names.index("drs_classifier_loss_region")
        adds = [c[1][0] for c in calls if c[0] == "drs_dice_loss_add"]
        assert len(adds) == 1 + (dice is not None) + (lov is not None) and adds[-1] == e.surface_loss_terms.data_ptr()
        for name in ("params", "mom", "grads", "bn"):
            assert torch.equal(getattr(a, name), getattr(e, name)), name
        assert torch.equal(oa["loss_parts"], oe["loss_parts"]) and torch.equal(a.region_grad[:M * K], e.region_grad[:M * K])
        if lov is None:
            g, _, pl = loops.surface_loss_grad(a.logits[:M * K].view(B, S, S, K), a.labels[:M].view(B, S, S), SURF[0], SURF[1],
                                               valid=a.acc_mask[:M].view(B, S, S),
                                               dice_coef=None if dice is None else a.dice_coef[:B * K * 2].view(B, K, 2))
            assert torch.equal(g.reshape(-1), a.region_grad[:M * K]) and torch.equal(pl, a.surface_loss_terms[:B])


def test_bad_values_are_rejected_by_both_nets():
    from drs_amd.net import DilatedNet
    nets = [DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV), DilatedNet("dilated_grsl", 5, 6, 0.005, b_max=1, s_max=9, device=DEV, engine=False)]
    for d in nets:
        for bad in (-1, 65, float("nan"), float("inf"), (1, 0.5), (1, 40000), (1, 2, 3), "2", True):
            with pytest.raises(ValueError):
                d.set_surface_loss(bad)
        assert d.surface_loss is None
        d.set_surface_loss((0.1, 5))
        assert d.surface_loss == (0.1, 5.0)
        d.set_surface_loss(0.2)
        assert d.surface_loss == (0.2, 0.0)
        d.set_surface_loss(None)
        assert d.surface_loss is None


# ------------------------------------------------------------------------------------------------- two ranks
# The spawn pattern and the bounds of tests/test_gpu_dice_loss.py::test_two_rank_step_follows_the_single_rank_step (those of
# tests/test_gpu_dp.py: loss 1e-6 ABSOLUTE, gradients 2e-3, parameters 1e-4), on that test's inputs.
DP = ("dilated8_grsl", 5, 6, 4, 21)
DP_SURF = (0.25, 8.0)


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
    loops.setup_surface_loss(d, DP_SURF, comm, lambda *a: None)          # what the loops do: one agree on the bits of the pair
    d.feed(x[sl], y[sl], S)
    res = d.train_step(B // world, S, 0.01)
    torch.cuda.synchronize()
    np.savez(out + "_rank%d.npz" % rank, grads=d.grads.cpu().numpy(), params=d.params.cpu().numpy(), bn=d.bn.cpu().numpy(),
             loss=d.loss_value(res["loss_parts"]), conf=res["conf"].cpu().numpy(), pair=np.asarray(d.surface_loss))
    comm.barrier()
    dist.destroy_process_group()


def test_two_rank_step_follows_the_single_rank_step(tmp_path):
    from drs_amd.net import DilatedNet
    NET, CH, K, B, S = DP
    out = str(tmp_path) + "/dp"
    mp.spawn(_dp_worker, args=(2, 32800 + os.getpid() % 1000, out), nprocs=2, join=True)
    x, y = _dp_inputs()
    losses = {}
    for s in (None, DP_SURF):                # (the step without the term too, to show below that it mattered)
        d = DilatedNet(NET, CH, K, 0.005, b_max=B, s_max=S, device=DEV, seed=3)
        d.set_surface_loss(s)
        d.feed(x, y, S)
        res = d.train_step(B, S, 0.01)
        torch.cuda.synchronize()
        losses[s] = d.loss_value(res["loss_parts"])
    r0, r1 = np.load(out + "_rank0.npz"), np.load(out + "_rank1.npz")
    assert tuple(r0["pair"]) == tuple(r1["pair"]) == DP_SURF
    loss = losses[DP_SURF]
    print("two ranks: loss %.9g (rank 0 %.9g), without the surface term %.9g" % (loss, float(r0["loss"]), losses[None]))
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
def test_train_loop_prints_the_combined_loss_and_keeps_the_pair(tmp_path, capsys, monkeypatch):
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
        seen.append((self.logits[:M * K].cpu().numpy().astype(np.float64).reshape(B, S, S, K), self.labels[:M].cpu().numpy().reshape(B, S, S),
                     out["loss_parts"].cpu().numpy().copy(), self.acc_mask[:M].cpu().numpy().reshape(B, S, S), kw.get("use_acc_mask", True)))
        return out
    monkeypatch.setattr(EngineNet, "train_step", recording)
    out = str(tmp_path) + "/"
    net = loops.train(data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 4, WD, mean, std, "loss", "single_fixed",
                      [13], None, None, None, None, 20, out, 1, "dilated_grsl", "vaihingen", "none", device=DEV,
                      val_cache_dir=str(tmp_path), surface_loss=(1.5, 4))
    text = capsys.readouterr().out
    assert "Surface loss: lambda 1.5 clip 4" in text and "Focal loss" not in text and "Dice term" not in text and "Lovasz" not in text
    assert net.surface_loss == (1.5, 4.0) and net.focal_gamma == 0.0 and net.dice is None and net.lovasz is None
    printed = [float(v) for v in re.findall(r"Training Minibatch: Loss= ([0-9.eE+-]+)", text)]
    assert len(printed) == len(seen) == 4
    for got, (lg, lab, parts, acc, use_acc) in zip(printed, seen):
        ce = focal_closed_form(lg.reshape(-1, K), lab.reshape(-1).astype(np.int64), np.ones(K), 0.0)["ce"]
        sv = SR.surface_loss(lg, lab, K, 1.5, 4.0, valid=acc if use_acc else None, inv_n=1.0 / lab.size)
        want = float(ce.mean()) + sv["loss"] + WD * float(parts[1])
        plain = float(ce.mean()) + WD * float(parts[1])
        print("loop loss printed %.6f combined %.6f cross-entropy %.6f" % (got, want, plain))
        assert abs(got - want) < 1e-4 * min(1.0, abs(want)) and abs(plain - want) > 1e-2 * plain
    assert os.path.isfile(out + "surface_loss_step_4.npy") and not os.path.exists(out + "lovasz_step_4.npy")
    assert np.load(out + "surface_loss_step_4.npy").tolist() == [1.5, 4.0]
    # a resumed run trains the same loss and says so; a pair given on a resumed run replaces the restored one, and the log says that too
    args = (data, labels, dist, rot, data, labels, dist, ["a", "b"], 0.01, 8, 5, WD, mean, std, "loss", "single_fixed", [13], None, None, None,
            None, 20, out, 1, "dilated_grsl", "vaihingen", out + "model-4")
    net2 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path))
    text = capsys.readouterr().out
    assert "Surface loss (restored from " + out + "surface_loss_step_4.npy): lambda 1.5 clip 4" in text and net2.surface_loss == (1.5, 4.0)
    net3 = loops.train(*args, device=DEV, val_cache_dir=str(tmp_path), surface_loss=2, focal_gamma=2.0)
    text = capsys.readouterr().out
    assert "Surface loss: lambda 2 clip none" in text and "replacing the pair restored from the checkpoint, lambda 1.5 clip 4" in text
    assert "Focal loss: gamma 2" in text and net3.surface_loss == (2.0, 0.0) and net3.focal_gamma == 2.0


def test_the_three_command_lines_take_the_option(tmp_path, monkeypatch, capsys):
    """one smoke per flavour, at the shapes of tests/test_gpu_loops.py's command-line tests"""
    from drs_amd import cli
    monkeypatch.chdir(tmp_path)           # the reference keeps its .npy caches in the cwd
    out = str(tmp_path) + "/out_"
    random.seed(0)
    np.random.seed(0)
    net = cli.main(["isprs_dilated_random.py", "--surface-loss=1.5,8", "synthetic:70x80x5/vaihingen/", out, "none", "a,b", "c", "0.01", "0.005",
                    "4", "2", "25", "10", "dilated8_grsl", "multi_fixed", "9,13", "acc", "training"], device=DEV)
    assert net.global_step == 2 and net.surface_loss == (1.5, 8.0) and os.path.isfile(out + "surface_loss_step_2.npy")
    net = cli.main_coffee(["coffee_dilated_random.py", "synthetic:2x60x60x3/", "synthetic:1x60x60x3/", out, "none", "0.01", "0.001", "6",
                           "2", "25", "10", "dilated_icpr_rate6_small", "multi_fixed", "9,13", "loss", "--surface-loss=0.5"], device=DEV)
    assert net.plan.K == 2 and net.global_step == 2 and net.surface_loss == (0.5, 0.0)
    net = cli.main_contest(["contest_dilated_random.py", "synthetic:80x70x3/", out, "none", "0.01", "0.001", "4", "2", "25", "10",
                            "dilated_grsl", "multi_fixed", "9,13", "acc", "train", "--surface-loss=2,5", "--lovasz-weight=1", "--dice-weight=1"],
                           device=DEV)
    assert net.plan.K == 7 and net.global_step == 2 and net.surface_loss == (2.0, 5.0) and net.lovasz == 1.0 and net.dice == (1.0, 0.5, 0.5, 1.0)
