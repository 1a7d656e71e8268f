"""-m gpu: the exact-fp32 convolution at channel widths that span SEVERAL column tiles.

include/drs.h promises "cout a multiple of 32 (>= 32)"; the nets only ever launch widths of one column tile (two at 256), where a
kernel that takes the tile width for a filter-row stride, output stride, statistics stride, bias offset or stream-K tile index gives
the right answer all the same.  Here every N tile of the forward / input-gradient and filter-gradient kernels runs three to nine
wide, on M = 3 * 10 * 10 = 300 pixels (two ragged 256-row, three ragged 128-row M tiles), against the fp64 oracle with the bound,
slab layout and guard rows of gpu_util.check_conv_forward_dgrad_wgrad (test_gpu_ops.py::test_conv_forward_dgrad_wgrad), and the
kernel forms (register-staged / LDS-DMA, halo-tap skipping, stream-K cuts) against each other bit for bit.

Every row names the tile grid it is there for and asserts it (drs_conv_mtile, drs_debug_wgrad_cut): a later change of the tile
rule fails the row instead of silently testing something else."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nets as onets

pytestmark = pytest.mark.gpu

from gpu_util import (DEV, GUARD, check_conv_forward_dgrad_wgrad, conv_case, conv_stats_moments, dev, guard_intact, guarded, padded,   # noqa: E402
                      rel_err, stream)

B, S = 3, 10
M = B * S * S


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


def _wgrad_grid(B, S, k, rate, cin, cout):
    """(tile rows, column tiles) of drs_conv_wgrad's launch of this shape, by the library's own cut (development library)"""
    from drs_amd import _lib
    d = _lib.dev()
    cap, tr = 1 << 14, ctypes.c_int(0)
    cut = np.zeros(5 * cap, dtype=np.int32)
    n = d.drs_debug_wgrad_cut(B, S, k, rate, onets.same_pad(k, rate)[0], cin, cout, cut.ctypes.data, cap, None, ctypes.addressof(tr))
    assert 0 < n <= cap
    return tr.value, int(cut[1:5 * n:5].max()) + 1


# (k, rate, cin, cout) -> (forward M tile, forward column tiles x width, filter-gradient (row tile, column tiles))
WIDTHS = {
    (3, 2, 32, 96): (256, (3, 32), (128, 3)),       # 3 x 32
    (3, 2, 32, 160): (256, (5, 32), (128, 5)),      # 5 x 32
    (3, 2, 64, 320): (128, (5, 64), (128, 5)),      # 5 x 64
    (3, 2, 64, 448): (128, (7, 64), (128, 7)),      # 7 x 64
    (3, 2, 64, 384): (128, (3, 128), (128, 3)),     # 3 x 128
    (3, 2, 64, 576): (128, (3, 192), (128, 3)),     # 3 x 192 (the LDS-DMA form: the only one of that width); 9 x 64 register-staged, below
    (4, 3, 64, 320): (128, (5, 64), (128, 5)),      # 5 x 64 under the even kernel: pad_before = 4 != pad_after = 5
    # the transposed problems: their INPUT gradient is the launch with N = cin (no bias, no statistics, the flipped filter)
    (3, 2, 96, 32): (256, (1, 32), (128, 1)),       # input gradient 3 x 32
    (3, 2, 160, 32): (256, (1, 32), (128, 1)),      # input gradient 5 x 32
    (3, 2, 224, 64): (128, (1, 64), (128, 1)),      # input gradient 7 x 32
    (3, 2, 448, 64): (128, (1, 64), (128, 1)),      # input gradient 7 x 64
    (3, 2, 384, 32): (256, (1, 32), (128, 1)),      # input gradient 3 x 128
    (3, 2, 576, 32): (256, (1, 32), (128, 1)),      # input gradient 3 x 192
}


def _tile_width(cout):
    """the N tile of the forward / input-gradient launch at its default form (pick_conv_tile, csrc/conv_mfma.hip)"""
    return 192 if cout % 192 == 0 and cout % 128 else (128 if cout % 128 == 0 else (64 if cout % 64 == 0 else 32))


@pytest.mark.parametrize("k,rate,cin,cout", list(WIDTHS))
def test_widths_forward_accumulate_dgrad_wgrad(lib, k, rate, cin, cout):
    mtile, (ncol, width), wgrid = WIDTHS[(k, rate, cin, cout)]
    assert lib.query("drs_conv_mtile", cout) == mtile and M % mtile != 0
    assert (cout // _tile_width(cout), _tile_width(cout)) == (ncol, width)
    assert _wgrad_grid(B, S, k, rate, cin, cout) == wgrid
    pb, pa = onets.same_pad(k, rate)
    assert (pb != pa) == (k == 4)
    check_conv_forward_dgrad_wgrad(lib, k, rate, cin, cout, B, S)


def test_widths_packed_taps_three_column_tiles(lib):
    """cin = 8 (5 bands in an 8-channel slab, drs_filter_pad_cin: four taps share a K-step) at cout = 96 = 3 x 32: the packed-tap
    kernel's filter rows are cout wide, not tile wide.  Filter gradient: 72 rows in one ragged row tile, 3 column tiles of 32."""
    k, rate, cin, cout, c_real = 3, 2, 8, 96, 5
    assert lib.query("drs_conv_mtile", cout) == 256
    assert _wgrad_grid(B, S, k, rate, cin, cout)[1] == 3
    check_conv_forward_dgrad_wgrad(lib, k, rate, cin, cout, B, S, c_real=c_real)


# ------------------------------------------------------------------------------------------------------------------ kernel forms
FORMS = [(3, 2, 64, 320), (3, 2, 64, 384), (3, 2, 64, 576)]       # 5 x 64, 3 x 128, 3 x 192 (9 x 64 register-staged)


def _operands(k, rate, cin, cout):
    c = conv_case(k, rate, cin, cout, B, S)
    pb, pa = onets.same_pad(k, rate)
    P = max(pb, pa)
    return c, pb, pa, P, padded(c["x"], P), padded(c["g"], P), dev(c["w"]), dev(c["bias"])


def _forward_wgrad(lib, k, rate, cin, cout, pb, P, xd, gd, wd, bd, mt):
    """forward with bias and tile statistics + filter gradient, every output with guard rows"""
    rows = -(-M // mt)
    out = guarded(M, cout, -3.0, mt)
    stats = guarded(rows, cout * 2, 0.0, 2)
    lib.call("drs_conv_forward", xd.data_ptr(), B, S, P, cin, 0, wd.data_ptr(), bd.data_ptr(), k, rate, pb, cin, cout, out.data_ptr(), cout, 0, 0,
             stats.data_ptr(), stream())
    nsp = lib.query("drs_conv_wgrad_splits", B, S, k, cin, cout)
    slab = guarded(nsp * k * k * cin, cout, 0.0, 128)
    gw = guarded(k * k * cin, cout, 7.0, 128)
    lib.call("drs_conv_wgrad", xd.data_ptr(), B, S, P, cin, 0, gd.data_ptr(), P, cout, 0, k, rate, pb, cin, cin, cout, slab.data_ptr(),
             gw.data_ptr(), stream())
    torch.cuda.synchronize()
    assert guard_intact(out, M) and guard_intact(stats, rows) and guard_intact(slab, nsp * k * k * cin) and guard_intact(gw, k * k * cin)
    return out[:M], stats[:rows], gw[:k * k * cin], nsp


def _oracle_errors(lib, c, res, mt, cout):
    out, stats, gw = res[:3]
    r2 = c["ref"].reshape(-1, cout)
    st = conv_stats_moments(lib, stats.contiguous(), M, mt, cout)
    return (rel_err(out.cpu().numpy(), r2), float(np.abs(st[:, 0] - r2.sum(axis=0)).max() / np.abs(r2).sum(axis=0).max()),
            rel_err(st[:, 1], (r2 ** 2).sum(axis=0)), rel_err(gw.cpu().numpy().reshape(c["gw_ref"].shape), c["gw_ref"]))


@pytest.mark.parametrize("k,rate,cin,cout", FORMS)
def test_widths_register_staged_and_lds_dma_forms(lib, k, rate, cin, cout):
    """as test_gpu_ops.py::test_register_staged_and_lds_dma_kernel_forms_are_bitwise_equal, several column tiles wide: the two forms of
    the forward (bias, statistics) and filter-gradient tiles bit for bit, and the product library's pick.  cout = 576 tiles
    differently in the two forms (3 x 192 LDS-DMA, 9 x 64 register-staged; asserted): each is held to the oracle, and the
    product library, which takes the 192-wide tile, to the LDS-DMA form."""
    from drs_amd import _lib as prod
    d = lib.dev()
    c, pb, pa, P, xd, gd, wd, bd = _operands(k, rate, cin, cout)
    mt = d.query("drs_conv_mtile", cout)
    assert mt == 128
    res, grids = {}, {}
    try:
        for v in (0, 1):
            d.drs_debug_conv_variant(v)
            d.drs_debug_wgrad_variant(v)
            grids[v] = _wgrad_grid(B, S, k, rate, cin, cout)
            res[v] = _forward_wgrad(d, k, rate, cin, cout, pb, P, xd, gd, wd, bd, mt)
    finally:
        d.drs_debug_conv_variant(-1)
        d.drs_debug_wgrad_variant(-1)
    if cout == 576:
        assert grids == {0: (128, 9), 1: (128, 3)}
    else:
        assert grids[0] == grids[1] == WIDTHS[(k, rate, cin, cout)][2]
        assert res[0][3] == res[1][3]
        for a, b, what in zip(res[0][:3], res[1][:3], ("fwd", "stats", "wgrad")):
            assert torch.equal(a, b), what
    for v in (0, 1):
        e = _oracle_errors(d, c, res[v], mt, cout)
        print("cout %d variant %d: fwd %.2e stats sum %.2e sq %.2e wgrad %.2e" % ((cout, v) + e))
        assert max(e) < 1e-5, (v, e)
    pres = _forward_wgrad(prod, k, rate, cin, cout, pb, P, xd, gd, wd, bd, mt)
    assert pres[3] == res[1][3]
    for a, b, what in zip(pres[:3], res[1][:3], ("fwd", "stats", "wgrad")):
        assert torch.equal(a, b), "product library, " + what


@pytest.mark.parametrize("k,rate,cin,cout", FORMS)
def test_widths_halo_tap_skipping_is_bitwise_neutral(lib, k, rate, cin, cout):
    """as test_gpu_ops.py::test_halo_tap_skipping_is_bitwise_neutral: the skip forced on (2) and off (0) gives the same bits in the
    forward, input-gradient and filter-gradient launches of the exact-fp32 and the split-bf16 kernels, several column tiles wide;
    the product library (its own rule) gives those bits too."""
    from drs_amd import _lib as prod
    d = lib.dev()
    c, pb, pa, P, xd, gd, wd, bd = _operands(k, rate, cin, cout)
    nw, ns = c["w"].size, 2
    wt = torch.zeros(nw, dtype=torch.float32, device=DEV)
    d.call("drs_filter_flip_transpose", wd.data_ptr(), wt.data_ptr(), k, cin, cout, stream())
    xt = torch.zeros(ns * xd.numel(), dtype=torch.int16, device=DEV)
    gt = torch.zeros(ns * gd.numel(), dtype=torch.int16, device=DEV)
    d.call("drs_split_terms", xd.data_ptr(), xd.numel(), ns, xt.data_ptr(), stream())
    d.call("drs_split_terms", gd.data_ptr(), gd.numel(), ns, gt.data_ptr(), stream())
    wf = torch.zeros(ns * nw, dtype=torch.int16, device=DEV)
    wg = torch.zeros(ns * nw, dtype=torch.int16, device=DEV)
    d.call("drs_filter_split", wd.data_ptr(), k, cin, cin, cout, ns, wf.data_ptr(), wg.data_ptr(), stream())

    def run(L, split):
        out = guarded(M, cout, -3.0, 128)
        gx = guarded(M, cin, -3.0, 128)
        gw = guarded(k * k * cin, cout, 7.0, 128)
        L.call("drs_conv_forward", xd.data_ptr(), B, S, P, cin, 0, wd.data_ptr(), None, k, rate, pb, cin, cout, out.data_ptr(), cout, 0, 0, None, stream())
        L.call("drs_conv_forward", gd.data_ptr(), B, S, P, cout, 0, wt.data_ptr(), None, k, rate, pa, cout, cin, gx.data_ptr(), cin, 0, 0, None, stream())
        nsp = L.query("drs_conv_wgrad_splits", B, S, k, cin, cout)
        slab = guarded(nsp * k * k * cin, cout, 0.0, 128)
        L.call("drs_conv_wgrad", xd.data_ptr(), B, S, P, cin, 0, gd.data_ptr(), P, cout, 0, k, rate, pb, cin, cin, cout, slab.data_ptr(), gw.data_ptr(),
               stream())
        outs = [out, gx, gw, slab]
        if split:
            out2 = guarded(M, cout, -3.0, 128)
            gx2 = guarded(M, cin, -3.0, 128)
            gw2 = guarded(k * k * cin, cout, 7.0, 128)
            L.call("drs_conv_forward_split", xt.data_ptr(), B, S, P, cin, 0, wf.data_ptr(), None, k, rate, pb, cin, cout, out2.data_ptr(), cout, 0, 0, None,
                   ns, stream())
            L.call("drs_conv_forward_split", gt.data_ptr(), B, S, P, cout, 0, wg.data_ptr(), None, k, rate, pa, cout, cin, gx2.data_ptr(), cin, 0, 0, None,
                   ns, stream())
            nsp2 = L.query("drs_conv_wgrad_split_splits", B, S, k, cin, cout, P, ns)
            slab2 = guarded(nsp2 * k * k * cin, cout, 0.0, 128)
            L.call("drs_conv_wgrad_split", xt.data_ptr(), B, S, P, cin, 0, gt.data_ptr(), P, cout, 0, k, rate, pb, cin, cin, cout, slab2.data_ptr(),
                   gw2.data_ptr(), ns, stream())
            outs += [out2, gx2, gw2, slab2]
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t[-2:] == GUARD).all())             # (the guard rows: every tensor here ends in at least 128 of them)
        return [t.cpu().numpy() for t in outs[:3] + outs[4:7]]
    res = {}
    try:
        for mode in (0, 2):
            d.drs_debug_skip_taps(mode)
            res[mode] = run(d, True)
    finally:
        d.drs_debug_skip_taps(1)
    names = ("fwd", "dgrad", "wgrad", "fwd split", "dgrad split", "wgrad split")
    for a, b, name in zip(res[0], res[2], names):
        np.testing.assert_array_equal(a, b, err_msg=name)
    e = (rel_err(res[2][0][:M], c["conv"].reshape(M, cout)), rel_err(res[2][1][:M], c["gx_ref"].reshape(M, cin)),
         rel_err(res[2][2][:k * k * cin].reshape(c["gw_ref"].shape), c["gw_ref"]))
    print("cout %d skip on: fwd %.2e dgrad %.2e wgrad %.2e" % ((cout,) + e))
    assert max(e) < 1e-5, e
    for a, b, name in zip(run(prod, False), res[0][:3], names):
        np.testing.assert_array_equal(a, b, err_msg="product library, " + name)


def _ws(lib, cout):
    n = lib.query("drs_conv_workspace_floats", cout)
    return torch.full((max(n, 1),), float("nan"), device=DEV), n          # poisoned: a piece read before it is written shows


@pytest.mark.parametrize("k,rate,cin,cout", FORMS)
def test_widths_streamk_cuts(lib, k, rate, cin, cout):
    """drs_conv_forward_ws with a NaN-poisoned workspace, several column tiles wide (the stream-K tile index -> (M tile, column tile)):
    the product library's own rule, then forced cuts W in {1, 2, tiles - 1, tiles, tiles + 1, U - 1, U} (tiles and U as
    test_gpu_streamk.py::test_streamk_every_cut_matches_oracle works them out, with the real tile width), each against the oracle
    with bias, statistics and the foreign channels of a wider output; bit for bit the plain kernel where no tile is cut."""
    from drs_amd import _lib as prod
    d = lib.dev()
    c, pb, pa, P, xd, gd, wd, bd = _operands(k, rate, cin, cout)
    ref = c["ref"]
    r2 = ref.reshape(-1, cout)
    mt = d.query("drs_conv_mtile", cout)
    bn = _tile_width(cout)
    assert mt == 128 and (cout // bn, bn) == WIDTHS[(k, rate, cin, cout)][1]
    tiles = -(-M // 128) * (cout // bn)
    nks = k * k * cin // 32
    U = tiles * nks
    rows = -(-M // mt)
    st = stream()

    def check(L, out, stats, tag):
        got = out.cpu().numpy()[:M]
        assert np.all(got[:, :32] == -3.0), tag
        assert guard_intact(out, M) and guard_intact(stats, rows), tag
        sv = conv_stats_moments(L, stats, M, mt, cout)
        e = (rel_err(got[:, 32:].reshape(ref.shape), ref), float(np.abs(sv[:, 0] - r2.sum(0)).max() / np.abs(r2).sum(0).max()),
             rel_err(sv[:, 1], (r2 ** 2).sum(0)))
        print("cout %d %s: fwd %.2e stats sum %.2e sq %.2e" % ((cout, tag) + e))
        assert max(e) < 1e-5, (tag, e)

    def launch(L, ws, nws, bias=True, out=None):
        out = guarded(M, cout + 32, -3.0, 128) if out is None else out
        stats = guarded(rows, cout * 2, 0.0, 2)
        L.call("drs_conv_forward_ws", xd.data_ptr(), B, S, P, cin, 0, wd.data_ptr(), bd.data_ptr() if bias else None, k, rate, pb, cin, cout,
               out.data_ptr(), cout + 32, 32, 0 if bias else 1, stats.data_ptr() if bias else None, ws.data_ptr(), nws, st)
        torch.cuda.synchronize()
        return out, stats
    plain = guarded(M, cout, -3.0, 128)
    pstats = guarded(rows, cout * 2, 0.0, 2)
    d.call("drs_conv_forward", xd.data_ptr(), B, S, P, cin, 0, wd.data_ptr(), bd.data_ptr(), k, rate, pb, cin, cout, plain.data_ptr(), cout, 0, 0,
           pstats.data_ptr(), st)
    # the product library under its own rule, and the development library at its default: the same bits
    pws, pnws = _ws(prod, cout)
    ws, nws = _ws(d, cout)
    assert pnws == nws and nws % (2 * 128 * bn) == 0 and nws > 0          # whole pieces of this tile: two per workgroup
    pout, pst = launch(prod, pws, pnws)
    check(prod, pout, pst, "product rule")
    d.drs_debug_conv_splitk(-1)
    dout, dst = launch(d, ws, nws)
    assert torch.equal(pout, dout) and torch.equal(pst, dst)
    whole = [W for W in range(1, tiles + 1) if U % W == 0 and (U // W) % nks == 0]
    try:
        for W in sorted({1, 2, tiles - 1, tiles, tiles + 1, U - 1, U}):
            d.drs_debug_conv_splitk(W)
            ws.fill_(float("nan"))
            out, stats = launch(d, ws, nws)
            check(d, out, stats, "W = %d" % W)
            if W in whole:               # no tile is cut: the same K order per tile as the plain kernel, bit for bit
                assert torch.equal(out[:M, 32:], plain[:M]) and torch.equal(stats, pstats), W
            # accumulate on top, no bias
            ws.fill_(float("nan"))
            out, _ = launch(d, ws, nws, bias=False, out=out)
            got = out.cpu().numpy()[:M]
            assert np.all(got[:, :32] == -3.0) and guard_intact(out, M), W
            assert rel_err(got[:, 32:].reshape(ref.shape), ref + c["conv"]) < 1e-5, W
    finally:
        d.drs_debug_conv_splitk(-1)


@pytest.mark.parametrize("k,rate,cin,cout", [(3, 2, 32, 96), (3, 2, 32, 160)])
def test_widths_32_wide_tiles_take_no_workspace(lib, k, rate, cin, cout):
    """the 256 x 32 tile has no stream-K form: drs_conv_workspace_floats is 0 and drs_conv_forward_ws, handed a (poisoned) workspace
    all the same, is the plain launch bit for bit"""
    c, pb, pa, P, xd, gd, wd, bd = _operands(k, rate, cin, cout)
    assert _tile_width(cout) == 32 and lib.query("drs_conv_workspace_floats", cout) == 0
    mt = lib.query("drs_conv_mtile", cout)
    rows = -(-M // mt)
    res = []
    ws = torch.full((1 << 16,), float("nan"), device=DEV)
    for with_ws in (False, True):
        out = guarded(M, cout, -3.0, mt)
        stats = guarded(rows, cout * 2, 0.0, 2)
        if with_ws:
            lib.call("drs_conv_forward_ws", xd.data_ptr(), B, S, P, cin, 0, wd.data_ptr(), bd.data_ptr(), k, rate, pb, cin, cout, out.data_ptr(), cout, 0, 0,
                     stats.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        else:
            lib.call("drs_conv_forward", xd.data_ptr(), B, S, P, cin, 0, wd.data_ptr(), bd.data_ptr(), k, rate, pb, cin, cout, out.data_ptr(), cout, 0, 0,
                     stats.data_ptr(), stream())
        torch.cuda.synchronize()
        res.append((out, stats))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(torch.isnan(ws).all())
    assert rel_err(res[1][0].cpu().numpy()[:M], c["ref"].reshape(M, cout)) < 1e-5
