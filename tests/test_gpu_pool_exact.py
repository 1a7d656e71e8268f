"""-m gpu: the two sliding kernels of the pooled nets (csrc/pointwise.hip: bn_act_pool_fwd_slide_kernel, bn_bwd_reduce_slide_kernel)
and the gathering forms that take over above 512 channels, held to EXACT bits and codes on every strip geometry.

Inputs come from tests/pool_exact_ref.py: a grid on which every fp32 operation of both kernels is exact (whatever the summation order,
with or without FMA contraction) and on which a quarter of all pooling windows hold a tie for the maximum, most of them at a positive
value.  The fp64 reference is then the required bit pattern of `out` and `gxhat`, the required code at every element, and the required
value of every row of the backward slab -- the one freedom being the sign of a zero maximum over zeros of both signs (see the
reference's docstring).  Every output buffer is poison-filled before the launches, `out` is a channel slice of a wider slab with a
halo, and the gradient is read from a slice.

The geometry of a launch (strips per image, rows per strip) follows slide_cfg and its two development switches
(drs_debug_slide_blocks, drs_debug_slide_minrows), which are statics of the development library's copy of pointwise.hip: every call
here goes through that one handle.  Each case first asks the library which geometry it will run (drs_bn_backward_rows) and fails if
that is not the one the case was written for; tests/test_pool_exact_plan.py holds the table to the classes it claims.
"""
import numpy as np
import pytest
import torch

import pool_exact_ref as R

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, stream   # noqa: E402

NAN_BITS = 0x7FC00000          # torch.full(nan)


@pytest.fixture()
def dev_lib():
    from drs_amd import _lib
    d = _lib.dev()
    old = (d.drs_debug_slide_blocks(-1), d.drs_debug_slide_minrows(-1))
    assert old == (R.SLIDE_BLOCKS, R.SLIDE_MINROWS)          # the library's defaults are the restated rule's
    try:
        yield d
    finally:
        d.drs_debug_slide_blocks(old[0])
        d.drs_debug_slide_minrows(old[1])


def _set(d, switches):
    blocks, minrows = switches
    d.drs_debug_slide_blocks(R.SLIDE_BLOCKS if blocks is None else blocks)
    d.drs_debug_slide_minrows(R.SLIDE_MINROWS if minrows is None else minrows)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expected_rows(d, shape, switches, want=None):
    """the geometry the library will run, read back from it, against the restated rule (and the case's claim)"""
    B, S, C = shape
    geo = R.case_geometry(shape, switches)
    rows = d.query("drs_bn_backward_rows", B, S, C, 1)
    if geo is None:
        assert want is None
        per = 256
        while per > 32 and (B * S * S) // per < 2048:          # bn_bwd_rows_per_block
            per >>= 1
        assert rows == -(-B * S * S // per)
        return rows, None
    assert rows % (B * geo["ncol"]) == 0 and rows // (B * geo["ncol"]) == geo["nstrips"], (rows, R.describe(geo))
    if want is not None:
        live = [n for n in geo["rows"] if n]
        assert (geo["nstrips"], geo["rps"], live[-1], geo["empty"]) == want
    return rows, geo


class _Run(object):
    """one forward + backward launch pair on poisoned buffers"""

    def __init__(self, d, zd, mrd, gad, ld_ga, coff_ga, B, S, C, alpha, P, ld, coff, rows, finish=None):
        M, Sp = B * S * S, S + 2 * P
        self.out = torch.full((B, Sp, Sp, ld), float("nan"), dtype=torch.float32, device=DEV)
        self.idx = torch.full((M * C,), 0xFF, dtype=torch.uint8, device=DEV)
        self.gxh = torch.full((M * C,), float("nan"), dtype=torch.float32, device=DEV)
        self.partial = torch.full((rows, C, 2), float("nan"), dtype=torch.float32, device=DEV)
        self.sums = torch.full((2 * C,), float("nan"), dtype=torch.float64, device=DEV)
        scr = torch.zeros(d.query("drs_colsum_scratch_doubles", 2 * C), dtype=torch.float64, device=DEV)
        if finish is None:
            d.call("drs_bn_act_pool_forward", zd.data_ptr(), B, S, C, mrd.data_ptr(), alpha, 1, self.out.data_ptr(), P, ld, coff,
                   self.idx.data_ptr(), stream())
        else:
            sums, mm, mv = finish
            d.call("drs_bn_finish_act_pool_forward", sums.data_ptr(), float(M), mrd.data_ptr(), mm.data_ptr(), mv.data_ptr(), 0.999, 1,
                   zd.data_ptr(), B, S, C, alpha, 1, self.out.data_ptr(), P, ld, coff, self.idx.data_ptr(), stream())
        d.call("drs_bn_backward_reduce", gad.data_ptr(), ld_ga, coff_ga, zd.data_ptr(), self.idx.data_ptr(), B, S, C, mrd.data_ptr(),
               alpha, 1, self.gxh.data_ptr(), self.partial.data_ptr(), stream())
        d.call("drs_stats_reduce", self.partial.data_ptr(), rows, C, self.sums.data_ptr(), scr.data_ptr(), stream())
        torch.cuda.synchronize()


def _check_view(full, S, P, coff, C):
    """[B,Sp,Sp,ld] numpy: the halo of the slice is +0.0, the channels beside it still hold the poison; -> the interior"""
    u = full.view(np.uint32)
    assert np.all(u[..., :coff] == NAN_BITS) and np.all(u[..., coff + C:] == NAN_BITS)
    sl = u[..., coff:coff + C]
    for halo in (sl[:, :P], sl[:, P + S:], sl[:, :, :P], sl[:, :, P + S:]):
        assert halo.size and not halo.any()
    return full[:, P:P + S, P:P + S, coff:coff + C]


@pytest.mark.parametrize("name,shape,switches,alpha,want", R.CASES, ids=[c[0] for c in R.CASES])
def test_exact_bits_and_codes(dev_lib, name, shape, switches, alpha, want):
    d = dev_lib
    B, S, C = shape
    M = B * S * S
    _set(d, switches)
    rows, geo = _expected_rows(d, shape, switches, want)
    print("\n%s %s @ %s alpha %s: %s, slab rows %d" % (name, shape, switches, alpha, R.describe(geo), rows))
    z, mr, g = R.exact_inputs(B, S, C, seed=S * 1000 + C)
    ref = R.reference(z, mr, alpha, g)
    P, ld, coff, ld_ga, coff_ga = 1 + S % 2, C + 8, 4, C + 16, 12
    gslab = np.full((M, ld_ga), 1e30, dtype=np.float32)          # beside the slice: would wreck every sum
    gslab[:, coff_ga:coff_ga + C] = g.reshape(M, C)
    run = _Run(d, dev(z.reshape(M, C)), dev(mr), dev(gslab), ld_ga, coff_ga, B, S, C, alpha, P, ld, coff, rows)

    got = _check_view(run.out.cpu().numpy(), S, P, coff, C)
    free = ref["zero_free"]
    want_out = ref["out"].astype(np.float32)
    assert np.array_equal(want_out.astype(np.float64), ref["out"])
    assert np.array_equal(_bits(got)[~free], _bits(want_out)[~free])
    assert np.all(got[free] == 0)
    idx = run.idx.cpu().numpy().reshape(B, S, S, C)
    assert np.array_equal(idx, ref["idx"]), "%d wrong codes" % int((idx != ref["idx"]).sum())
    gxh = run.gxh.cpu().numpy().reshape(B, S, S, C)
    assert np.array_equal(_bits(gxh), _bits(ref["gxhat"].astype(np.float32)))

    partial = run.partial.cpu().numpy().astype(np.float64)
    assert np.isfinite(partial).all()                                # every row written
    if geo is not None:
        slab = R.slide_partials(ref["gxhat"], ref["xhat"], geo)
        assert slab.shape == partial.shape
        assert np.array_equal(partial, slab)                         # row by row; the rows of empty strips are zero
        if geo["empty"]:
            p5 = partial.reshape(B, geo["nstrips"], geo["ncol"], C, 2)
            assert not p5[:, geo["nstrips"] - geo["empty"]:].any() and p5[:, :geo["nstrips"] - geo["empty"]].any()
    sums = run.sums.cpu().numpy().reshape(C, 2)
    assert np.array_equal(sums[:, 0], ref["sum_g"]) and np.array_equal(sums[:, 1], ref["sum_gx"])
    assert np.abs(ref["sum_gx"]).max() > 0


def test_geometries_agree_on_ordinary_data(dev_lib):
    """random normal data, statistics from drs_bn_finish, alpha = 0.1, one shape under three geometries: out, idx and gxhat have the
    same bits in all of them; the folded finish (drs_bn_finish_act_pool_forward) gives the bits of drs_bn_finish +
    drs_bn_act_pool_forward in each; out and idx are the bits of the same chain in numpy fp32 (a subtraction, a product, maxima: no
    order and no contraction to differ by); gxhat and the two sums agree with fp64"""
    d = dev_lib
    B, S, C = R.INVARIANCE_SHAPE
    M, alpha = B * S * S, 0.1
    gen = torch.Generator(device=DEV).manual_seed(17)
    zd = torch.randn(M, C, device=DEV, generator=gen) * 1.5 + 0.3
    ld_ga, coff_ga = C + 16, 12
    gad = torch.randn(M, ld_ga, device=DEV, generator=gen)
    z64 = zd.double()
    sums = torch.stack([z64.sum(0), (z64 * z64).sum(0)], dim=1).reshape(-1).contiguous()
    del z64

    def finish_buffers():
        return (torch.full((2 * C,), float("nan"), device=DEV), torch.linspace(-1, 1, C, device=DEV), torch.linspace(0.5, 2, C, device=DEV))

    mr, mm, mv = finish_buffers()
    d.call("drs_bn_finish", sums.data_ptr(), float(M), C, mr.data_ptr(), mm.data_ptr(), mv.data_ptr(), 0.999, 1, stream())
    torch.cuda.synchronize()
    assert torch.isfinite(mr).all()
    P, ld, coff = 2, C + 8, 4
    runs = []
    for sw in R.INVARIANCE_SETTINGS:
        _set(d, sw)
        rows, geo = _expected_rows(d, (B, S, C), sw)
        print("\n%s @ %s: %s, slab rows %d" % ((B, S, C), sw, R.describe(geo), rows))
        run = _Run(d, zd, mr, gad, ld_ga, coff_ga, B, S, C, alpha, P, ld, coff, rows)
        mr2, mm2, mv2 = finish_buffers()
        fused = _Run(d, zd, mr2, gad, ld_ga, coff_ga, B, S, C, alpha, P, ld, coff, rows, finish=(sums, mm2, mv2))
        for a, b in ((run.out, fused.out), (mr, mr2), (mm, mm2), (mv, mv2), (run.gxh, fused.gxh), (run.partial, fused.partial)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(run.idx, fused.idx)
        runs.append((geo, run))
    assert [g["rows"] for g, r in runs] == [[17], [9, 8], [5, 5, 5, 2]]
    first = runs[0][1]
    for geo, run in runs[1:]:
        assert torch.equal(run.out.view(torch.int32), first.out.view(torch.int32))
        assert torch.equal(run.idx, first.idx)
        assert torch.equal(run.gxh.view(torch.int32), first.gxh.view(torch.int32))

    z = zd.cpu().numpy().reshape(B, S, S, C)
    g = gad[:, coff_ga:coff_ga + C].cpu().numpy().reshape(B, S, S, C)
    mrh = mr.cpu().numpy().reshape(C, 2)
    r32 = R.reference(z, mrh, alpha, dtype=np.float32)
    got = _check_view(first.out.cpu().numpy(), S, P, coff, C)
    assert not r32["zero_free"].any()
    assert np.array_equal(_bits(got), _bits(r32["out"]))
    idx = first.idx.cpu().numpy().reshape(B, S, S, C)
    assert np.array_equal(idx, r32["idx"])
    # backward in fp64 along the codes just checked
    xhat = (z.astype(np.float64) - mrh[:, 0].astype(np.float64)) * mrh[:, 1].astype(np.float64)
    assert np.array_equal(xhat > 0, r32["xhat"] > 0)
    gpool = R.pool_backward(idx, g.astype(np.float64))
    gx = np.where(xhat > 0, gpool, gpool * alpha)
    gxh = first.gxh.cpu().numpy().reshape(B, S, S, C).astype(np.float64)
    assert np.abs(gxh - gx).max() <= 1e-6 * np.abs(gx).max()
    s1, s2 = gx.sum(axis=(0, 1, 2)), (gx * xhat).sum(axis=(0, 1, 2))
    b1, b2 = 1e-6 * np.abs(gx).sum(axis=(0, 1, 2)), 1e-6 * np.abs(gx * xhat).sum(axis=(0, 1, 2))
    for geo, run in runs:
        sm = run.sums.cpu().numpy().reshape(C, 2)
        e1, e2 = np.abs(sm[:, 0] - s1) / b1, np.abs(sm[:, 1] - s2) / b2
        print("%s: sums off by %.3f / %.3f of the bound" % (geo["rows"], e1.max(), e2.max()))
        assert e1.max() <= 1.0 and e2.max() <= 1.0
