"""-m gpu: the entry points of include/drs.h that test_gpu_ops.py does not call -- average pool, squeeze-and-excitation (forward
and backward), the term-writing forms of the batch-norm kernels, `pool` bit 1 of drs_bn_act_pool_forward, drs_softmax_accumulate
and drs_scale_f64 -- each against the fp64 oracle (oracle/tf_ops.py) or a numpy fp64 statement of the same operation, at the
smallest shapes that reach each code path of the kernels.  Tolerance: test_gpu_ops.py's single-op bar, 1e-5 of the reference
tensor's maximum magnitude; integer outputs and comparisons called bitwise are exact.  (An fp32 numpy restatement of these ops
against the oracle stays below 8.1e-7 on every shape listed here.)  Every comparison prints its observed error (-s)."""
import numpy as np
import pytest
import torch

from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, rel_err, stream, unpad   # noqa: E402
from test_gpu_split import split_host                   # noqa: E402

BAR = 1e-5
NAN_TERM = 0x7FC0          # a bf16 quiet NaN: what a term buffer holds where no kernel has written


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


def _show(what, case, **errs):
    print("\n%-12s %-34s %s" % (what, case, "  ".join("%s %.2e" % (k, v) for k, v in errs.items())), end="", flush=True)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _slab(B, S, P, ld, fill=5.0):
    return torch.full((B * (S + 2 * P) ** 2 * ld,), fill, dtype=torch.float32, device=DEV)


def _check_view(out, B, S, P, ld, coff, C, fill=5.0):
    """interior of the slice; asserts that its halo is exactly zero and that the channels beside it still hold `fill`"""
    got, full = unpad(out, B, S, P, ld, coff, C)
    halo = full[:, :, :, coff:coff + C].copy()
    halo[:, P:P + S, P:P + S] = 0
    assert np.all(halo == 0)
    assert np.all(full[:, :, :, :coff] == fill) and np.all(full[:, :, :, coff + C:] == fill)
    return got


# ------------------------------------------------------------------------------------------------ 1. average pool
AVG_CASES = [
    (64, 5, 2, 13, 3, 96, 32),       # the net's own shape, written into a slice
    (256, 7, 2, 9, 6, 256, 0),       # k = 7 at the widest channel count
    (128, 7, 1, 5, 2, 128, 0),       # window clipped on both sides at every pixel
    (64, 5, 2, 2, 0, 64, 0),         # k > S and P_out == 0: no halo launch
    (4, 3, 3, 1, 1, 8, 4),           # one pixel, one channel quad
    (100, 9, 1, 6, 1, 104, 4),       # C / 4 = 25: the e / CQ split is ragged
    (576, 3, 1, 20, 1, 576, 0),      # 2880 work items per row: several x-blocks and a ragged last one
    (64, 1, 1, 8, 2, 64, 0),         # k = 1
]


def _avg_device(lib, x, g, k, P, ld, coff):
    """drs_avg_pool_forward of x into a 5.0-filled slab and drs_avg_pool_backward of g, read as a slice (ld C + 16, coff 16) of a
    slab with junk beside it, into a junk-filled gin"""
    B, S, _, C = x.shape
    M = B * S * S
    out = _slab(B, S, P, ld)
    lib.call("drs_avg_pool_forward", dev(x.reshape(M, C)).data_ptr(), B, S, C, k, out.data_ptr(), P, ld, coff, stream())
    gd = torch.full((M, C + 16), -7.5, dtype=torch.float32, device=DEV)
    gd[:, 16:] = dev(g.reshape(M, C))
    gin = torch.full((M * C,), 11.0, dtype=torch.float32, device=DEV)
    lib.call("drs_avg_pool_backward", gd.data_ptr(), C + 16, 16, B, S, C, k, gin.data_ptr(), stream())
    torch.cuda.synchronize()
    return out, gin.cpu().numpy().reshape(B, S, S, C)


@pytest.mark.parametrize("C,k,B,S,P,ld,coff", AVG_CASES)
def test_avg_pool_forward_backward(lib, C, k, B, S, P, ld, coff):
    rng = np.random.default_rng([1, C, k, B, S, P])
    x = (rng.normal(size=(B, S, S, C)) * 1.5 + 0.3).astype(np.float32)
    g = rng.normal(size=(B, S, S, C)).astype(np.float32)
    ref, cnt = T.avg_pool_same(x.astype(np.float64), k)
    gref = T.avg_pool_same_bwd(g.astype(np.float64), k, cnt)
    out, gin = _avg_device(lib, x, g, k, P, ld, coff)
    got = _check_view(out, B, S, P, ld, coff, C)
    e_f, e_b = rel_err(got, ref), rel_err(gin, gref)
    # The adjoint identity <avg(x), g> == <x, avg_bwd(g)>, in fp64 from the device's own outputs: it fails if the divisors of the
    # two directions disagree at clipped borders, whatever the oracle says.  On strictly positive x and g, so that neither inner
    # product is a cancelling sum whose magnitude could fall by chance to that of its rounding error.
    xa, ga = np.abs(x) + np.float32(0.1), np.abs(g) + np.float32(0.1)
    outa, gina = _avg_device(lib, xa, ga, k, P, ld, coff)
    ya = unpad(outa, B, S, P, ld, coff, C)[0]
    lhs = float((ya.astype(np.float64) * ga.astype(np.float64)).sum())
    rhs = float((xa.astype(np.float64) * gina.astype(np.float64)).sum())
    e_a = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
    _show("avg_pool", (C, k, B, S, P, ld, coff), fwd=e_f, bwd=e_b, adjoint=e_a)
    assert e_f < BAR
    assert e_b < BAR
    assert e_a < BAR
    if k == 1:
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))        # a 1 x 1 window: the input, bit for bit


# ------------------------------------------------------------------------------------------------ 2. squeeze-and-excitation
SE_CASES = [
    (64, 16, 3, 9, 2, 96, 32),       # net shape, written into a slice
    (128, 32, 2, 14, 3, 128, 0),     # net shape
    (256, 64, 2, 33, 1, 256, 0),     # net shape
    (100, 25, 2, 5, 1, 104, 4),      # second channel group of 64 is partial; odd R
    (68, 17, 1, 7, 0, 68, 0),        # partial channel group and P_out == 0
    (320, 80, 1, 6, 0, 320, 0),      # C > 256: the excite kernels' loops stride past the block size
    (64, 3, 2, 6, 1, 64, 0),         # R not equal to C / 4
    (64, 16, 5, 1, 0, 64, 0),        # one pixel: three of the four pixel lanes are idle
    (64, 16, 2, 2, 1, 64, 0),        # four pixels
]
MARGIN = 1e-3


def _se_inputs(rng, C, R, B, S):
    """A ReLU-like activation (non-negative, non-zero mean), every value different per image, and the layer's parameters with
    every hidden unit's pre-activation kept MARGIN away from the ReLU's kink in the fp64 reference, so that the fp32 kernel takes
    the same branch and no element has to be left out of a comparison.  With R >= 3, unit 0 has a zero w1 column and a zero bias
    (pre-activation exactly 0 in both arithmetics) and unit 1 is dead (bias -10); neither goes through the margin adjustment.  Should no
    ordinary unit fire for any image (a few units, all drawn negative), the first one's bias is set so that it does."""
    act = np.maximum(rng.normal(size=(B, S, S, C)) * 1.5 + 0.3, 0).astype(np.float32)
    w1 = (rng.normal(size=(C, R)) / np.sqrt(C)).astype(np.float32)
    w2 = (rng.normal(size=(R, C)) / np.sqrt(R)).astype(np.float32)
    b1 = (0.5 * rng.normal(size=R)).astype(np.float32)
    b2 = (0.5 * rng.normal(size=C)).astype(np.float32)
    free = np.ones(R, dtype=bool)
    if R >= 3:
        w1[:, 0] = 0.0
        b1[0] = 0.0
        b1[1] = -10.0
        free[:2] = False
    s = act.astype(np.float64).mean(axis=(1, 2))
    j = int(np.argmax(free))
    if not ((s @ w1.astype(np.float64) + b1.astype(np.float64))[:, free] > MARGIN).any():
        b1[j] = np.float32(1.0 - (s @ w1.astype(np.float64))[:, j].min())       # at least one ordinary unit fires: dw1 / db1 are not all zero
    rounds = 0
    while True:
        pre1 = s @ w1.astype(np.float64) + b1.astype(np.float64)
        close = (np.abs(pre1) < MARGIN).any(axis=0) & free
        if not close.any():
            break
        b1[close] += np.float32(2 * MARGIN)
        rounds += 1
        assert rounds <= 3
    live = np.ones(R, dtype=bool)
    live[0] = R < 3                   # the constructed zero unit sits on the kink by design
    assert np.abs(pre1[:, live]).min() >= MARGIN
    if R >= 3:
        assert np.all(pre1[:, 0] == 0) and np.all(pre1[:, 1] < -MARGIN)
    return act, w1, b1, w2, b2


@pytest.mark.parametrize("C,R,B,S,P,ld,coff", SE_CASES)
def test_se_forward_backward(lib, C, R, B, S, P, ld, coff):
    rng = np.random.default_rng([2, C, R, B, S, P])
    M = B * S * S
    act, w1, b1, w2, b2 = _se_inputs(rng, C, R, B, S)
    gy = rng.normal(size=(B, S, S, C)).astype(np.float32)
    f64 = lambda a: a.astype(np.float64)      # noqa: E731
    ref, (s_ref, e1_ref, e2_ref) = T.se_forward(f64(act), f64(w1), f64(b1), f64(w2), f64(b2))
    gx_ref, gp_ref = T.se_backward(f64(act), (s_ref, e1_ref, e2_ref), f64(w1), f64(w2), f64(gy))

    actd, w1d, b1d, w2d, b2d = dev(act.reshape(M, C)), dev(w1), dev(b1), dev(w2), dev(b2)
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)      # noqa: E731
    s, e1, e2 = nan(B * C), nan(B * R), nan(B * C)
    out = _slab(B, S, P, ld)
    lib.call("drs_se_forward", actd.data_ptr(), B, S, C, R, w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(),
             s.data_ptr(), e1.data_ptr(), e2.data_ptr(), out.data_ptr(), P, ld, coff, stream())
    torch.cuda.synchronize()
    got = _check_view(out, B, S, P, ld, coff, C)
    e1h = e1.cpu().numpy().reshape(B, R)
    errs = dict(s=rel_err(s.cpu().numpy().reshape(B, C), s_ref), e1=rel_err(e1h, e1_ref),
                e2=rel_err(e2.cpu().numpy().reshape(B, C), e2_ref), out=rel_err(got, ref))

    # backward on the device's own s, e1, e2 (as the engine runs it), gy read as a slice of a wider slab with junk beside it,
    # every output prefilled with junk (overwritten, not added to), twice on the same buffers (fixed order, no atomics: same bits)
    gyd = torch.full((M, C + 32), 3.25, dtype=torch.float32, device=DEV)
    gyd[:, 32:] = dev(gy.reshape(M, C))
    scratch = nan(B * (3 * C + R))
    outs = [torch.full((n,), -6.5, dtype=torch.float32, device=DEV) for n in (M * C, C * R, R, R * C, C)]
    first = None
    for _ in range(2):
        lib.call("drs_se_backward", gyd.data_ptr(), C + 32, 32, actd.data_ptr(), s.data_ptr(), e1.data_ptr(), e2.data_ptr(), w1d.data_ptr(),
                 w2d.data_ptr(), B, S, C, R, *[t.data_ptr() for t in outs], scratch.data_ptr(), stream())
        torch.cuda.synchronize()
        if first is None:
            first = [_bits(t).copy() for t in outs]
    for a, t, what in zip(first, outs, ("gact", "dw1", "db1", "dw2", "db2")):
        assert np.array_equal(a, _bits(t)), what
    gact, dw1, db1, dw2, db2 = [t.cpu().numpy() for t in outs]
    dw1, dw2 = dw1.reshape(C, R), dw2.reshape(R, C)
    errs.update(gact=rel_err(gact.reshape(B, S, S, C), gx_ref), dw1=rel_err(dw1, gp_ref["w1"]), db1=rel_err(db1, gp_ref["b1"]),
                dw2=rel_err(dw2, gp_ref["w2"]), db2=rel_err(db2, gp_ref["b2"]))
    _show("se", (C, R, B, S, P, ld, coff), **errs)
    for what, e in errs.items():
        assert e < BAR, what
    if R >= 3:       # the unit that sits exactly on the kink passes no gradient (relu'(0) = 0, as tf.nn.relu's gradient)
        assert np.all(e1h[:, 0] == 0)
        assert np.all(dw1[:, 0] == 0) and db1[0] == 0
        assert np.all(e1h[:, 1] == 0)
    if B == 1:       # drs_se_scale_const with that gate is the same kernel with another gate stride: the same bits
        out2 = _slab(B, S, P, ld)
        lib.call("drs_se_scale_const", actd.data_ptr(), B, S, C, e2.data_ptr(), out2.data_ptr(), P, ld, coff, stream())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out2), _bits(out))


# ------------------------------------------------------------------------------------------------ 3. term-writing BN kernels
TERM_CASES = [(64, 1, 0.1, 2, 9, 4, 2), (128, 0, 0.0, 2, 7, 6, 3), (192, 1, 0.1, 1, 12, 0, 2), (32, 1, 0.1, 2, 5, 2, 3),
              (256, 0, 0.0, 3, 10, 6, 3), (576, 1, 0.1, 1, 5, 1, 2)]


def _bn_inputs(lib, rng, C, B, S):
    """z and mean_rstd as test_gpu_ops.test_bn_act_pool_forward_backward makes them, its exact tie of two maxima included"""
    M = B * S * S
    z = (rng.normal(size=(B, S, S, C)) * 1.5 + 0.3).astype(np.float32)
    if S >= 2:
        z[0, 0, 0, :] = z[0, 0, 1, :] = 10.0
    return z, dev(z.reshape(M, C)), _mean_rstd(lib, z.reshape(M, C))


def _mean_rstd(lib, z2):
    M, C = z2.shape
    part = np.stack([z2.sum(axis=0), (z2.astype(np.float64) ** 2).sum(axis=0)], axis=1).astype(np.float32)
    sums = torch.zeros(C * 2, dtype=torch.float64, device=DEV)
    scr = torch.zeros(lib.query("drs_colsum_scratch_doubles", 2 * C), dtype=torch.float64, device=DEV)
    lib.call("drs_stats_reduce", dev(part.reshape(1, C, 2)).data_ptr(), 1, C, sums.data_ptr(), scr.data_ptr(), stream())
    mr = torch.zeros(C * 2, dtype=torch.float32, device=DEV)
    lib.call("drs_bn_finish", sums.data_ptr(), float(M), C, mr.data_ptr(), None, None, 0.999, 1, stream())
    return mr


def _term_buf(n, ns):
    return torch.full((ns * n,), NAN_TERM, dtype=torch.int16, device=DEV)


def _by_term(a, ns):
    """[ns * n] in the kernels' layout (term s of element e at (e & ~31) * ns + 32 s + (e & 31)) -> [ns][n]"""
    n = a.size // ns
    return a.reshape(n // 32, ns, 32).transpose(1, 0, 2).reshape(ns, n)


def _decode(t, ns):
    return _by_term(t.view(torch.bfloat16).to(torch.float32).cpu().numpy(), ns)


def _check_terms(lib, terms, slab, ns, B, S, P, ld, coff, C):
    """the terms of the slice, halo included, are the host split of the fp32 slab term by term; halo terms are 0; terms of the
    channels beside the slice still hold the prefill; with ld == C the buffer is what drs_split_terms makes of the whole slab"""
    Sp = S + 2 * P
    shape = (B, Sp, Sp, ld)
    got = _decode(terms, ns)
    raw = _by_term(terms.cpu().numpy().view(np.uint16), ns)
    want = split_host(slab.cpu().numpy(), ns)
    for t in range(ns):
        g4, w4, r4 = got[t].reshape(shape), want[t].reshape(shape), raw[t].reshape(shape)
        assert np.array_equal(g4[..., coff:coff + C], w4[..., coff:coff + C]), t
        halo = g4[..., coff:coff + C].copy()
        halo[:, P:P + S, P:P + S] = 0
        assert np.all(halo == 0), t
        assert np.all(r4[..., :coff] == NAN_TERM) and np.all(r4[..., coff + C:] == NAN_TERM), t
    if ld == C:
        whole = torch.zeros(ns * slab.numel(), dtype=torch.int16, device=DEV)
        lib.call("drs_split_terms", slab.data_ptr(), slab.numel(), ns, whole.data_ptr(), stream())
        torch.cuda.synchronize()
        assert np.array_equal(_decode(whole, ns), got)


@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "slice"])
@pytest.mark.parametrize("C,pool,alpha,B,S,P,ns", TERM_CASES)
def test_bn_term_writing_forms(lib, C, pool, alpha, B, S, P, ns, sliced):
    """drs_bn_act_pool_forward_terms / drs_bn_backward_apply_terms against the plain entry points (bitwise: for pooled C <= 512 that
    holds the gathering kernel to the sliding one, both "first maximum in scan order" on the same fp32 values) and against the host's
    statement of the term split."""
    rng = np.random.default_rng(C + S)
    M = B * S * S
    ld, coff = (C + 32, 32) if sliced else (C, 0)
    n = B * (S + 2 * P) ** 2 * ld
    z, zd, mr = _bn_inputs(lib, rng, C, B, S)
    ga = rng.normal(size=(M, C)).astype(np.float32)
    idx_ptr = lambda t: t.data_ptr() if pool else None      # noqa: E731
    new_idx = lambda: torch.full((M * C,), 77, dtype=torch.uint8, device=DEV)      # noqa: E731

    out_a, idx_a = _slab(B, S, P, ld), new_idx()
    lib.call("drs_bn_act_pool_forward", zd.data_ptr(), B, S, C, mr.data_ptr(), alpha, pool, out_a.data_ptr(), P, ld, coff, idx_ptr(idx_a), stream())
    out_b, idx_b, terms_b = _slab(B, S, P, ld), new_idx(), _term_buf(n, ns)
    lib.call("drs_bn_act_pool_forward_terms", zd.data_ptr(), B, S, C, mr.data_ptr(), alpha, pool, out_b.data_ptr(), P, ld, coff, idx_ptr(idx_b),
             terms_b.data_ptr(), ns, stream())
    idx_c, terms_c = new_idx(), _term_buf(n, ns)
    lib.call("drs_bn_act_pool_forward_terms", zd.data_ptr(), B, S, C, mr.data_ptr(), alpha, pool, None, P, ld, coff, idx_ptr(idx_c),
             terms_c.data_ptr(), ns, stream())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out_b), _bits(out_a))
    assert torch.equal(idx_b, idx_a) and torch.equal(idx_c, idx_a)
    _check_view(out_a, B, S, P, ld, coff, C)
    _check_terms(lib, terms_b, out_a, ns, B, S, P, ld, coff, C)
    assert torch.equal(terms_c, terms_b)
    if pool:        # bit 1 (the caller vouches for the halo, here after a call on other values): the same slab and terms
        z_other = dev(np.ascontiguousarray(z[:, ::-1]).reshape(M, C))
        out_d, idx_d, terms_d = _slab(B, S, P, ld), new_idx(), _term_buf(n, ns)
        for zz, pl in ((z_other, 1), (zd, 3)):
            lib.call("drs_bn_act_pool_forward_terms", zz.data_ptr(), B, S, C, mr.data_ptr(), alpha, pl, out_d.data_ptr(), P, ld, coff,
                     idx_d.data_ptr(), terms_d.data_ptr(), ns, stream())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out_d), _bits(out_a)) and torch.equal(terms_d, terms_b) and torch.equal(idx_d, idx_a)

    # backward: gxhat and the two sums as test_bn_act_pool_forward_backward makes them
    gad = torch.zeros(M, C + 16, dtype=torch.float32, device=DEV)
    gad[:, 16:] = dev(ga)
    gxh = torch.zeros(M * C, dtype=torch.float32, device=DEV)
    rows = lib.query("drs_bn_backward_rows", B, S, C, pool)
    partial = torch.zeros(rows * C * 2, dtype=torch.float32, device=DEV)
    lib.call("drs_bn_backward_reduce", gad.data_ptr(), C + 16, 16, zd.data_ptr(), idx_ptr(idx_a), B, S, C, mr.data_ptr(), alpha, pool,
             gxh.data_ptr(), partial.data_ptr(), stream())
    bs = torch.zeros(C * 2, dtype=torch.float64, device=DEV)
    scr = torch.zeros(lib.query("drs_colsum_scratch_doubles", 2 * C), dtype=torch.float64, device=DEV)
    lib.call("drs_stats_reduce", partial.data_ptr(), rows, C, bs.data_ptr(), scr.data_ptr(), stream())
    apply_args = (gxh.data_ptr(), zd.data_ptr(), B, S, C, mr.data_ptr(), bs.data_ptr(), float(M))
    gz_a = _slab(B, S, P, ld)
    lib.call("drs_bn_backward_apply", *apply_args, gz_a.data_ptr(), P, ld, coff, stream())
    gz_b, gt_b, gt_c = _slab(B, S, P, ld), _term_buf(n, ns), _term_buf(n, ns)
    lib.call("drs_bn_backward_apply_terms", *apply_args, gz_b.data_ptr(), P, ld, coff, gt_b.data_ptr(), ns, stream())
    lib.call("drs_bn_backward_apply_terms", *apply_args, None, P, ld, coff, gt_c.data_ptr(), ns, stream())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(gz_b), _bits(gz_a))
    got = _check_view(gz_a, B, S, P, ld, coff, C)
    assert np.abs(got).max() > 0
    _check_terms(lib, gt_b, gz_a, ns, B, S, P, ld, coff, C)
    assert torch.equal(gt_c, gt_b)


# ------------------------------------------------------------------------------------------------ 4. pool bit 1
@pytest.mark.parametrize("C,B,S,P", [(64, 2, 9, 4), (448, 1, 7, 3),       # the sliding form, which leaves the halo to its own launch
                                     (576, 1, 5, 1), (64, 2, 9, 0)])      # the gathering form above 512 channels; no halo at all
def test_pool_bit_1_leaves_a_zero_halo_alone(lib, C, B, S, P):
    """pool = 3 on a slab whose halo a pool = 1 call with the same B, S, P has zeroed: interior and positions are those of a
    pool = 1 call on a fresh slab, the halo is still zero, the channels beside the slice untouched."""
    rng = np.random.default_rng(C * 3 + S)
    M = B * S * S
    ld, coff = C + 8, 4
    z1 = (rng.normal(size=(M, C)) * 2.0 - 0.4).astype(np.float32)
    z2, z2d, mr = _bn_inputs(lib, rng, C, B, S)
    used, idx_u = _slab(B, S, P, ld), torch.full((M * C,), 77, dtype=torch.uint8, device=DEV)
    for zz, pl in ((dev(z1), 1), (z2d, 3)):
        lib.call("drs_bn_act_pool_forward", zz.data_ptr(), B, S, C, mr.data_ptr(), 0.1, pl, used.data_ptr(), P, ld, coff, idx_u.data_ptr(), stream())
    fresh, idx_f = _slab(B, S, P, ld), torch.full((M * C,), 77, dtype=torch.uint8, device=DEV)
    lib.call("drs_bn_act_pool_forward", z2d.data_ptr(), B, S, C, mr.data_ptr(), 0.1, 1, fresh.data_ptr(), P, ld, coff, idx_f.data_ptr(), stream())
    torch.cuda.synchronize()
    got = _check_view(used, B, S, P, ld, coff, C)
    want = _check_view(fresh, B, S, P, ld, coff, C)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert torch.equal(idx_u, idx_f)
    assert np.abs(want).max() > 0 and int(idx_f.max()) <= 8          # (the fresh call did write)


# ------------------------------------------------------------------------------------------------ 5. softmax accumulate, scale
@pytest.mark.parametrize("h,w,K", [(7, 5, 1), (33, 41, 6), (19, 23, 8),
                                   (1100, 1000, 2)])     # more pixels than the launch's 4096 x 256 threads: the grid-stride loop
def test_softmax_accumulate(lib, h, w, K):
    rng = np.random.default_rng([5, h, w, K])
    occur = rng.integers(0, 6, size=(h, w)).astype(np.int32)
    occur[0, 0], occur[h - 1, w - 1] = 0, 5
    logits = rng.uniform(-20.0, 20.0, size=(h, w, K)).astype(np.float32)      # inside expf's range: no max subtraction (isprs:38-43)
    prob = (occur[..., None].astype(np.float32) * logits).astype(np.float32)
    acc0 = rng.uniform(0.0, 1.0, size=(h, w, K)).astype(np.float32)
    acc, probd, occd = dev(acc0), dev(prob), dev(occur)
    for _ in range(2):
        lib.call("drs_softmax_accumulate", probd.data_ptr(), occd.data_ptr(), h, w, K, acc.data_ptr(), stream())
    ones = torch.ones(h * w, dtype=torch.int32, device=DEV)
    lab = torch.full((h * w,), 255, dtype=torch.uint8, device=DEV)
    lib.call("drs_stitch_finalize", acc.data_ptr(), ones.data_ptr(), h, w, K, lab.data_ptr(), stream())
    torch.cuda.synchronize()
    e = np.exp(prob.astype(np.float64) / np.maximum(occur, 1)[..., None])
    ref = acc0.astype(np.float64) + 2.0 * e / e.sum(axis=-1, keepdims=True)
    err = rel_err(acc.cpu().numpy().reshape(h, w, K), ref)
    top = np.sort(ref, axis=-1)
    clear = (top[..., -1] - top[..., -2] > 1e-4) if K > 1 else np.ones((h, w), dtype=bool)
    _show("softmax_acc", (h, w, K), acc=err, clear=clear.mean())
    assert err < BAR
    assert clear.mean() > 0.9
    assert np.array_equal(lab.cpu().numpy().reshape(h, w)[clear], ref.argmax(axis=-1)[clear])


@pytest.mark.parametrize("n", [1, 4, 1000])
def test_scale_f64(lib, n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=n) * np.exp(rng.normal(size=n) * 3)
    s = 1.0 / 37.0
    xd = dev(x)
    lib.call("drs_scale_f64", xd.data_ptr(), n, s, stream())
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x * s)          # one IEEE multiplication either way
