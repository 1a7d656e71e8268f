"""Helpers for the -m gpu parity tests (device views <-> numpy NHWC)."""
import numpy as np
import torch

DEV = "cuda:0"


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def padded(x, P, ld=None, coff=0, fill=0.0):
    """numpy [B,S,S,C] -> device slab [B,S+2P,S+2P,ld] with x in channels coff.. and `fill` elsewhere in the
    interior's other channels / halo (fill != 0 lets a test see a kernel that forgets to zero the halo)."""
    B, S, _, C = x.shape
    ld = ld or C
    buf = np.full((B, S + 2 * P, S + 2 * P, ld), fill, dtype=np.float32)
    buf[:, :, :, coff:coff + C] = 0.0
    buf[:, P:P + S, P:P + S, coff:coff + C] = x
    return dev(buf)


def unpad(t, B, S, P, ld, coff, C):
    a = t.detach().cpu().numpy().reshape(B, S + 2 * P, S + 2 * P, ld)
    return a[:, P:P + S, P:P + S, coff:coff + C], a


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


GUARD = 1.0e30      # what guard rows hold: no sum of these tests comes near it


def guarded(rows, width, fill, guard_rows):
    """device [rows + guard_rows, width] float32: `fill` in the rows a kernel may write, GUARD in the rows after them (an overrun by a
    ragged last tile then fails guard_intact instead of faulting)"""
    t = torch.full((rows + guard_rows, width), float(fill), dtype=torch.float32, device=DEV)
    t[rows:] = GUARD
    return t


def guard_intact(t, rows):
    return bool((t[rows:] == GUARD).all())


def conv_case(k, rate, cin, cout, B, S, c_real=None):
    """the seeded operands of one convolution and its fp64 oracle results (oracle.tf_ops), computed once per shape and shared: treat
    as read-only.  c_real: the few-band input of conv1 -- c_real channels in a cin-wide (8 / 16) slab, no input gradient."""
    key = (k, rate, cin, cout, B, S, c_real)
    if key not in _CASES:
        from oracle import tf_ops as T
        c = c_real or cin
        rng = np.random.default_rng(k * 1000 + rate * 100 + cin + cout + S)
        x = rng.normal(size=(B, S, S, c)).astype(np.float32)
        w = (rng.normal(size=(k, k, c, cout)) / np.sqrt(k * k * c)).astype(np.float32)
        bias = rng.normal(size=(cout,)).astype(np.float32)
        g = rng.normal(size=(B, S, S, cout)).astype(np.float32)
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        conv = T.conv2d_same(x64, w64, rate)
        gx_ref, gw_ref = T.conv2d_same_bwd(x64, w64, rate, g.astype(np.float64))
        _CASES[key] = dict(x=x, w=w, bias=bias, g=g, conv=conv, ref=conv + bias.astype(np.float64), gx_ref=gx_ref, gw_ref=gw_ref)
    return _CASES[key]


_CASES = {}


def check_conv_forward_dgrad_wgrad(lib, k, rate, cin, cout, B, S, c_real=None):
    """drs_conv_forward (bias + tile statistics, then accumulate mode), the input gradient through drs_filter_flip_transpose and
    drs_conv_wgrad against the fp64 oracle, rel_err < 1e-5 of the tensor's maximum: the input a slice of a wider slab (ld = cin + 32,
    coff = 32, junk in the foreign channels), the output in (M, cout + 32) at coff = 32 with a sentinel in the foreign channels, a halo
    one wider than needed; output, statistics slab, input gradient and filter-gradient slab carry guard rows after their last used
    row, which must stay untouched.  Returns the measured errors."""
    from oracle import nets as onets
    c = conv_case(k, rate, cin, cout, B, S, c_real)
    x, w, bias, g, ref = c["x"], c["w"], c["bias"], c["g"], c["ref"]
    pb, pa = onets.same_pad(k, rate)
    P = max(pb, pa) + 1                      # a halo wider than needed must also work
    M = B * S * S
    if c_real:                               # the slab's own channels past the real ones are zero, as the crop leaves them
        x = np.concatenate([x, np.zeros((B, S, S, cin - c_real), dtype=np.float32)], axis=3)
    xd = padded(x, P, ld=cin + 32, coff=32, fill=7.0)      # slice of a wider slab; foreign channels are junk
    bd = dev(bias)
    if c_real:                               # packed taps: k*k*cin filter rows, padded with zero rows to a multiple of 32
        wd = torch.zeros(-(-k * k * cin // 32) * 32 * cout, dtype=torch.float32, device=DEV)
        lib.call("drs_filter_pad_cin", dev(w).data_ptr(), wd.data_ptr(), k, c_real, cin, cout, stream())
    else:
        wd = dev(w)
    mt = lib.query("drs_conv_mtile", cout)
    rows = (M + mt - 1) // mt
    out = guarded(M, cout + 32, -3.0, mt)
    stats = guarded(rows, cout * 2, 0.0, 2)
    lib.call("drs_conv_forward", xd.data_ptr(), B, S, P, cin + 32, 32, wd.data_ptr(), bd.data_ptr(), k, rate, pb, cin, cout,
             out.data_ptr(), cout + 32, 32, 0, stats.data_ptr(), stream())
    torch.cuda.synchronize()
    err = {}
    got = out.cpu().numpy()[:M]
    err["fwd"] = rel_err(got[:, 32:].reshape(B, S, S, cout), ref)
    assert err["fwd"] < 1e-5
    assert np.all(got[:, :32] == -3.0)                      # neighbouring channels untouched
    assert guard_intact(out, M) and guard_intact(stats, rows)
    st = conv_stats_moments(lib, stats, M, mt, cout)
    r2 = ref.reshape(-1, cout)
    err["stats_sum"] = float(np.abs(st[:, 0] - r2.sum(axis=0)).max() / np.abs(r2).sum(axis=0).max())
    err["stats_sq"] = rel_err(st[:, 1], (r2 ** 2).sum(axis=0))
    assert err["stats_sum"] < 1e-5
    assert err["stats_sq"] < 1e-5
    # accumulate mode
    lib.call("drs_conv_forward", xd.data_ptr(), B, S, P, cin + 32, 32, wd.data_ptr(), None, k, rate, pb, cin, cout,
             out.data_ptr(), cout + 32, 32, 1, None, stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:M]
    err["acc"] = rel_err(got[:, 32:].reshape(B, S, S, cout), ref + c["conv"])
    assert err["acc"] < 1e-5
    assert np.all(got[:, :32] == -3.0) and guard_intact(out, M)

    # gradients
    gd = padded(g, P, ld=cout, coff=0)
    gx = guarded(M, cin, 0.0, 256)
    if not c_real:
        wt = torch.zeros(k * k * cin * cout, dtype=torch.float32, device=DEV)
        lib.call("drs_filter_flip_transpose", wd.data_ptr(), wt.data_ptr(), k, cin, cout, stream())
        lib.call("drs_conv_forward", gd.data_ptr(), B, S, P, cout, 0, wt.data_ptr(), None, k, rate, pa, cout, cin, gx.data_ptr(),
                 cin, 0, 0, None, stream())
    nsplit = lib.query("drs_conv_wgrad_splits", B, S, k, cin, cout)
    slab = guarded(nsplit * k * k * cin, cout, 0.0, 128)
    gw = guarded(k * k * (c_real or cin), cout, 0.0, 128)
    lib.call("drs_conv_wgrad", xd.data_ptr(), B, S, P, cin + 32, 32, gd.data_ptr(), P, cout, 0, k, rate, pb, cin, c_real or cin, cout,
             slab.data_ptr(), gw.data_ptr(), stream())
    torch.cuda.synchronize()
    if not c_real:
        err["dgrad"] = rel_err(gx.cpu().numpy()[:M].reshape(B, S, S, cin), c["gx_ref"])
        assert err["dgrad"] < 1e-5
    err["wgrad"] = rel_err(gw.cpu().numpy()[:k * k * (c_real or cin)].reshape(c["gw_ref"].shape), c["gw_ref"])
    assert err["wgrad"] < 1e-5
    assert guard_intact(gx, M) and guard_intact(slab, nsplit * k * k * cin) and guard_intact(gw, k * k * (c_real or cin))
    print("k%d r%d %3d->%3d B%d S%d: " % (k, rate, c_real or cin, cout, B, S) + " ".join("%s %.2e" % kv for kv in err.items()))
    return err


def conv_stats_moments(lib, stats, M, mt, cout):
    """statistics slab of a convolution epilogue (per tile (sum, M2 about the tile mean)) -> numpy [cout, 2] = (sum z, sum z^2),
    through drs_conv_stats_reduce (Chan combination in fp64)."""
    sums = torch.zeros(2 * cout, dtype=torch.float64, device=DEV)
    lib.call("drs_conv_stats_reduce", stats.data_ptr(), M, mt, cout, sums.data_ptr(), None, stream())
    torch.cuda.synchronize()
    return sums.cpu().numpy().reshape(cout, 2)
