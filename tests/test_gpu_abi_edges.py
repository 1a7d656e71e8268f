"""-m gpu: corners INSIDE the argument domains of include/drs.h that no other test calls, each held to a plain reference.

a. drs_stitch_accumulate / drs_stitch_finalize at strides other than floor(S / 2), up to the limit of 5 regular windows per axis plus
   the shifted-back one, against oracle.host_ref.stitch_tile, bit for bit.
b. drs_tile_place (the plain copy form, which otherwise runs only inside whole-map tests) against a numpy copy, and the device-side box
   checks of both place kernels: a box outside the image or outside its tile places nothing.  The map lives inside a larger
   allocation with a guard band of T rows on both sides and no bad box is off by more than T, so that even a broken check could not
   write outside memory this test owns.
c. the view arguments of the filter gradients: Px != Pg, Pg = 0, coff_g != 0, ld_g > cout, on the ragged, the tracked and the affine
   pixel walk, against the fp64 filter gradient; the halo widths must not move a bit of the sums.
(tests/test_abi_contract.py holds what lies OUTSIDE the domains, on a machine without a device.)"""
import numpy as np
import pytest
import torch

from oracle import host_ref as H
from oracle import tf_ops as T

pytestmark = pytest.mark.gpu

from gpu_util import DEV, dev, padded, rel_err, stream   # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from drs_amd import _lib
    assert torch.cuda.is_available()
    _lib.load()
    return _lib


# ------------------------------------------------------------------------------------------------------------- a. stitching
# (h, w, S, stride, K, windows per call): the batch size never divides the windows of a row, so batches end mid-row
STITCH = [
    (70, 57, 25, 5, 6, 5),       # 5 regular windows over a pixel on one axis, 5 plus the shifted-back one on the other: the array limit
    (41, 40, 16, 4, 2, 5),       # an ordinary small stride
    (50, 48, 16, 16, 7, 5),      # stride = S: disjoint windows plus a shifted-back one
    (33, 40, 33, 16, 3, 3),      # a single window row
]


@pytest.mark.parametrize("h,w,S,stride,K,bs", STITCH)
def test_stitch_at_other_strides_matches_reference_order(lib, h, w, S, stride, K, bs):
    rng = np.random.default_rng(h * 100 + stride)
    nh, nw = H.window_counts(h, w, S, stride)
    assert nw % bs != 0 and (S + stride - 1) // stride <= 5
    tile, lab = np.zeros((h, w, 1)), np.zeros((h, w), dtype=np.uint8)
    prob = torch.zeros(h * w * K, dtype=torch.float32, device=DEV)
    occ = torch.zeros(h * w, dtype=torch.int32, device=DEV)
    batches, keep = [], []
    for i in range(-(-nh * nw // bs)):
        _, _, pos = H.create_patches_per_map(tile, lab, S, stride, i, bs)
        lg = rng.normal(size=(len(pos), S, S, K)).astype(np.float32)
        batches.append((lg, pos))
        keep.append(dev(lg))
        lib.call("drs_stitch_accumulate", prob.data_ptr(), occ.data_ptr(), keep[-1].data_ptr(), h, w, K, S, stride, i * bs, len(pos), stream())
    assert sum(len(pos) for _, pos in batches) == nh * nw
    out = torch.zeros(h * w, dtype=torch.uint8, device=DEV)
    lib.call("drs_stitch_finalize", prob.data_ptr(), occ.data_ptr(), h, w, K, out.data_ptr(), stream())
    torch.cuda.synchronize()
    p_ref, o_ref, am_ref = H.stitch_tile(h, w, K, S, batches)
    np.testing.assert_array_equal(occ.cpu().numpy().reshape(h, w), o_ref[:, :, 0])
    np.testing.assert_array_equal(prob.cpu().numpy().reshape(h, w, K), p_ref)      # same addition order: bit for bit
    np.testing.assert_array_equal(out.cpu().numpy().reshape(h, w), am_ref)


# ------------------------------------------------------------------------------------------------------------- b. placing tiles
PH, PW, PT, PK = 40, 52, 32, 6
SENTINEL = -123.25


def _plan():
    from drs_amd import patches as P
    boxes = P.dense_tiles(PH, PW, PT, 5, 6)
    assert len(boxes) == 4
    return boxes


def _bad_boxes():
    """every way a box can lie outside the image or outside its tile, none off by more than one pixel (the guard band is T rows)"""
    h, w, T_ = PH, PW, PT
    ok = (4, 10, 6, 30, 12, 40)                          # a good box (origin (4, 10), core inside the tile) that each row below breaks
    y0, x0, cy0, cy1, cx0, cx1 = ok
    bad = [
        (-1, x0, cy0, cy1, cx0, cx1), (y0, -1, cy0, cy1, cx0, cx1),                          # origin before the image
        (h - T_ + 1, x0, h - T_ + 3, h, cx0, cx1), (y0, w - T_ + 1, cy0, cy1, w - T_ + 3, w),      # tile past the image's end
        (y0, x0, y0 - 1, cy1, cx0, cx1), (y0, x0, cy0, y0 + T_ + 1, cx0, cx1),               # core outside its tile, each side
        (y0, x0, cy0, cy1, x0 - 1, cx1), (y0, x0, cy0, cy1, cx0, x0 + T_ + 1),
        (y0, x0, cy1, cy0, cx0, cx1), (y0, x0, cy0, cy1, cx1, cx0),                          # inverted core
        (y0, x0, cy0, cy0, cx0, cx1), (y0, x0, cy0, cy1, cx0, cx0),                          # empty core (a valid box that covers nothing)
    ]
    return np.asarray(bad, dtype=np.int64)


class _Guarded(object):
    """prob [h][w][K] and occur [h][w] inside larger allocations: a band of T rows' worth of elements on both sides, filled with a
    sentinel and checked afterwards"""

    def __init__(self, fill):
        self.gp, self.go = PT * PW * PK, PT * PW
        self.prob = torch.full((2 * self.gp + PH * PW * PK,), fill, dtype=torch.float32, device=DEV)
        self.occ = torch.full((2 * self.go + PH * PW,), 77, dtype=torch.int32, device=DEV)
        self.occ[self.go:self.go + PH * PW] = 0
        self.fill = fill

    def ptrs(self):
        return self.prob[self.gp:].data_ptr(), self.occ[self.go:].data_ptr()

    def read(self):
        p, o = self.prob.cpu().numpy(), self.occ.cpu().numpy()
        for band in (p[:self.gp], p[self.gp + PH * PW * PK:]):
            assert (band == np.float32(self.fill)).all(), "the guard band of prob was written"
        for band in (o[:self.go], o[self.go + PH * PW:]):
            assert (band == 77).all(), "the guard band of occur was written"
        return p[self.gp:self.gp + PH * PW * PK].reshape(PH, PW, PK), o[self.go:self.go + PH * PW].reshape(PH, PW)


def _mixed_boxes():
    """good boxes of the plan between the bad ones: (boxes [n][6], indices of the good ones)"""
    plan, bad = _plan(), _bad_boxes()
    rows, good = [], []
    for i, b in enumerate(bad):
        if i in (0, 6):
            good.append(len(rows))
            rows.append(plan[0 if i == 0 else 3])
        rows.append(b)
    return np.asarray(rows, dtype=np.int64), good


def test_tile_place_copies_every_core_and_counts_once(lib):
    boxes = _plan()
    n = len(boxes)
    rng = np.random.default_rng(11)
    logits = rng.normal(size=(n, PT, PT, PK)).astype(np.float32)
    lg, bx = dev(logits), dev(boxes.astype(np.int32))
    m = _Guarded(SENTINEL)
    pp, po = m.ptrs()
    lib.call("drs_tile_place", pp, po, lg.data_ptr(), PH, PW, PK, PT, bx.data_ptr(), n, stream())
    torch.cuda.synchronize()
    prob, occ = m.read()
    want = np.full((PH, PW, PK), SENTINEL, dtype=np.float32)
    for i, (y0, x0, cy0, cy1, cx0, cx1) in enumerate(boxes):
        want[cy0:cy1, cx0:cx1] = logits[i, cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    assert (want != SENTINEL).all()                                  # the cores partition the image
    np.testing.assert_array_equal(prob, want)
    assert (occ == 1).all()


def test_tile_place_bad_boxes_place_nothing(lib):
    boxes, good = _mixed_boxes()
    plan = _plan()
    # two more good boxes whose cores overlap: the tile of plan box 2 once more, with a part of that core and the same logits
    y0, x0, cy0, cy1, cx0, cx1 = plan[2]
    sub = (y0, x0, cy0 + 3, cy1 - 2, cx0 + 1, cx1 - 7)
    boxes = np.concatenate([boxes, np.asarray([plan[2], sub], dtype=np.int64)])
    good = good + [len(boxes) - 2, len(boxes) - 1]
    n = len(boxes)
    assert n == 12 + 2 + 2
    rng = np.random.default_rng(12)
    logits = rng.normal(size=(n, PT, PT, PK)).astype(np.float32)
    logits[-1] = logits[-2]
    lg, bx = dev(logits), dev(boxes.astype(np.int32))
    m = _Guarded(SENTINEL)
    pp, po = m.ptrs()
    lib.call("drs_tile_place", pp, po, lg.data_ptr(), PH, PW, PK, PT, bx.data_ptr(), n, stream())
    torch.cuda.synchronize()
    prob, occ = m.read()
    want = np.full((PH, PW, PK), SENTINEL, dtype=np.float32)
    cnt = np.zeros((PH, PW), dtype=np.int32)
    for i in good:
        y0, x0, cy0, cy1, cx0, cx1 = boxes[i]
        want[cy0:cy1, cx0:cx1] = logits[i, cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
        cnt[cy0:cy1, cx0:cx1] += 1
    assert cnt.max() == 2 and (cnt == 2).sum() == (sub[3] - sub[2]) * (sub[5] - sub[4]) and (cnt == 0).any()
    np.testing.assert_array_equal(occ, cnt)                          # bad boxes count nothing; the overlap counts twice
    np.testing.assert_array_equal(prob, want)                        # ... and leave the sentinel where no good core lies


def _softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


@pytest.mark.parametrize("g", [0, 5])
def test_tile_place_dihedral_bad_boxes_place_nothing(lib, g):
    from drs_amd import patches as P
    boxes, good = _mixed_boxes()                                     # (the good cores are disjoint, as this call requires)
    n = len(boxes)
    rng = np.random.default_rng(13 + g)
    logits = (rng.normal(size=(n, PT, PT, PK)) * 4).astype(np.float32)
    lg, bx = dev(logits), dev(boxes.astype(np.int32))
    base = 2.0
    m = _Guarded(base)
    pp, po = m.ptrs()
    lib.call("drs_tile_place_dihedral", pp, po, lg.data_ptr(), PH, PW, PK, PT, bx.data_ptr(), n, g, stream())
    torch.cuda.synchronize()
    acc, occ = m.read()
    (_, _), (Ii, Ji) = P.dihedral_index(g, PT)
    want = np.full((PH, PW, PK), base, dtype=np.float64)
    cnt = np.zeros((PH, PW), dtype=np.int32)
    for i in good:
        y0, x0, cy0, cy1, cx0, cx1 = boxes[i]
        back = _softmax(logits[i].astype(np.float64)[Ii, Ji])
        want[cy0:cy1, cx0:cx1] += back[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
        cnt[cy0:cy1, cx0:cx1] += 1
    assert cnt.max() == 1 and (cnt == 0).any()
    np.testing.assert_array_equal(occ, cnt)
    assert (acc[cnt == 0] == np.float32(base)).all()                 # untouched, bit for bit
    assert rel_err(acc, want) <= 1e-6                                # the bound of test_tile_place_dihedral_against_numpy


# ------------------------------------------------------------------------------------------------------------- c. filter-gradient views
CIN, COUT = 32, 64
LDX, CX, LDG, CG = CIN + 32, 32, COUT + 32, 32
HALOS = [(2, 0), (2, 5), (6, 2)]                 # (Px, Pg): independent; Pg = 0 has no halo pixel to read zeros from
TOL_F32 = 1e-5                                   # test_gpu_ops.py::test_conv_forward_dgrad_wgrad
TOL_SPLIT = {2: 1.6e-5, 3: 1e-5}                 # test_gpu_split.py::test_conv_split_forward_dgrad_wgrad (TOL there, with its derivation)


def _planes(lib, t, ns):
    n = t.numel()
    assert n % 32 == 0
    p = torch.zeros(ns * n, dtype=torch.int16, device=DEV)
    lib.call("drs_split_terms", t.data_ptr(), n, ns, p.data_ptr(), stream())
    return p


def _wgrads(lib, x, g, B, S, k, rate, pb, Px, Pg):
    """the filter gradient of the three arithmetics on views (Px, ld_x, coff_x) / (Pg, ld_g, coff_g): junk in the foreign channels,
    zeros in the halos; returns {0: fp32, 2: two terms, 3: three terms} as numpy [k][k][cin][cout]"""
    nw = k * k * CIN * COUT
    xd = padded(x, Px, ld=LDX, coff=CX, fill=7.0)
    gd = padded(g, Pg, ld=LDG, coff=CG, fill=7.0)
    out = {}
    slab = torch.zeros(lib.query("drs_conv_wgrad_splits", B, S, k, CIN, COUT) * nw, dtype=torch.float32, device=DEV)
    gw = torch.full((nw,), 3.0, dtype=torch.float32, device=DEV)
    lib.call("drs_conv_wgrad", xd.data_ptr(), B, S, Px, LDX, CX, gd.data_ptr(), Pg, LDG, CG, k, rate, pb, CIN, CIN, COUT,
             slab.data_ptr(), gw.data_ptr(), stream())
    torch.cuda.synchronize()
    out[0] = gw.cpu().numpy().reshape(k, k, CIN, COUT)
    for ns in (2, 3):
        xp, gp = _planes(lib, xd, ns), _planes(lib, gd, ns)
        slab = torch.zeros(lib.query("drs_conv_wgrad_split_splits", B, S, k, CIN, COUT, Pg, ns) * nw, dtype=torch.float32, device=DEV)
        gw = torch.full((nw,), 3.0, dtype=torch.float32, device=DEV)
        lib.call("drs_conv_wgrad_split", xp.data_ptr(), B, S, Px, LDX, CX, gp.data_ptr(), Pg, LDG, CG, k, rate, pb, CIN, CIN, COUT,
                 slab.data_ptr(), gw.data_ptr(), ns, stream())
        torch.cuda.synchronize()
        out[ns] = gw.cpu().numpy().reshape(k, k, CIN, COUT)
    return out


def _case(B, S, k):
    rng = np.random.default_rng(1000 * B + 10 * S + k)
    x = rng.normal(size=(B, S, S, CIN)).astype(np.float32)
    g = rng.normal(size=(B, S, S, COUT)).astype(np.float32)
    return x, g


# (B, S): M % 32 != 0 with the per-chunk set() path (S < 11); the tracked walk (S >= 11); the affine form (S % 32 == 0, no ragged chunk)
@pytest.mark.parametrize("B,S", [(2, 9), (2, 13), (1, 32)])
def test_wgrad_views_with_independent_halos(lib, B, S):
    k, rate = 3, 2
    pb, pa = 2, 2
    assert ((B * S * S) % 32 != 0) == (S != 32)
    x, g = _case(B, S, k)
    _, ref = T.conv2d_same_bwd(x.astype(np.float64), np.zeros((k, k, CIN, COUT)), rate, g.astype(np.float64))
    got = {}
    for Px, Pg in HALOS:
        assert Px >= max(pb, pa)
        got[(Px, Pg)] = _wgrads(lib, x, g, B, S, k, rate, pb, Px, Pg)
        for ns, gw in got[(Px, Pg)].items():
            e = rel_err(gw, ref)
            print("B %d S %2d Px %d Pg %d terms %d: wgrad %.2e" % (B, S, Px, Pg, ns, e))
            assert e < (TOL_SPLIT[ns] if ns else TOL_F32), (Px, Pg, ns, e)
    # halo widths must not move the sums: the cut of the pixels depends on the shape alone, and with Pg > 0 on both sides the split
    # form runs the same kernel (drs_conv_wgrad_split_splits takes Pg only to tell Pg == 0, the register-staged form, from Pg > 0)
    for ns in (0, 2, 3):
        np.testing.assert_array_equal(got[(2, 5)][ns], got[(6, 2)][ns], err_msg="terms %d" % ns)


def test_wgrad_views_1x1_without_halos(lib):
    B, S, k, rate = 2, 9, 1, 1
    x, g = _case(B, S, k)
    _, ref = T.conv2d_same_bwd(x.astype(np.float64), np.zeros((k, k, CIN, COUT)), rate, g.astype(np.float64))
    for ns, gw in _wgrads(lib, x, g, B, S, k, rate, 0, 0, 0).items():
        e = rel_err(gw, ref)
        print("1x1 B %d S %d terms %d: wgrad %.2e" % (B, S, ns, e))
        assert e < (TOL_SPLIT[ns] if ns else TOL_F32), (ns, e)
