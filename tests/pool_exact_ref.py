"""Exact reference of the pooled batch-norm kernels (csrc/pointwise.hip: drs_bn_act_pool_forward and drs_bn_backward_reduce with
pool = 1), numpy, independent of oracle/.

The chain is  xhat = (z - mean) * rstd;  a = max(alpha * xhat, xhat);  out, code = 3x3 max pool (stride 1, SAME; padding never wins;
code = 3 dy + dx of the FIRST maximum in window scan order);  backward: the incoming gradient of every output goes to the input its
code names, gx = xhat > 0 ? g : g * alpha, and per channel sum(gx), sum(gx * xhat).

`exact_inputs` draws inputs on which every fp32 operation of that chain is exact, whatever the summation order and with or without
FMA contraction:
  z      quarter integers k / 4, k in -6 .. 6; mean a quarter integer in -2/4 .. 2/4; rstd in {0.5, 1, 2}
         -> z - mean is a quarter integer, |.| <= 2; xhat a multiple of 1/8, |xhat| <= 4
  alpha  0 or 0.25 -> alpha * xhat a multiple of 1/32: exact; a maximum of exact values is exact
  g      integers -8 .. 8 -> at most nine of them meet in one input: an integer, |.| <= 72; times alpha a multiple of 1/4
  gx * xhat  a multiple of 1/32, |.| <= 288: a workgroup's sum over n pixels stays a multiple of 1/32 below 288 n, exact in fp32 while
         288 * 32 * n < 2^24, i.e. n < 1820 pixels per workgroup (`MAX_EXACT_PIXELS`; the test table stays below 400)
So the fp64 evaluation IS the bit pattern a correct fp32 kernel must give -- with one freedom: the sign of a zero maximum.  With
alpha = 0 a negative xhat becomes -0.0 and a zero xhat +0.0; C leaves fmaxf(-0.0, +0.0) to the implementation, and the two kernel forms
(fmaxf in the sliding kernel, `a > best` in the gathering one) do choose differently.  `reference` therefore reports `zero_free`: the
outputs whose window holds zeros of both signs as its maximum.  Everywhere else the sign of a zero is determined, and checked.

`slide_geometry` restates slide_cfg of pointwise.hip (the strip geometry of the two sliding kernels) so that a test can say which
geometry a shape reaches.
"""
import numpy as np

ALPHAS = (0.0, 0.25)
MAX_ABS_TERM = 288.0           # |gx * xhat| <= 72 * 4
TERM_UNIT = 1.0 / 32.0
MAX_EXACT_PIXELS = int(2 ** 24 * TERM_UNIT / MAX_ABS_TERM)      # 1820


def exact_inputs(B, S, C, seed=0):
    """(z [B,S,S,C] fp32, mean_rstd [C,2] fp32, g [B,S,S,C] fp32) on the exact grid of the module docstring"""
    rng = np.random.default_rng(seed)
    z = (rng.integers(-6, 7, size=(B, S, S, C), dtype=np.int8).astype(np.float32)) * np.float32(0.25)
    mean = rng.integers(-2, 3, size=C).astype(np.float32) * np.float32(0.25)
    rstd = np.array([0.5, 1.0, 2.0], dtype=np.float32)[rng.integers(0, 3, size=C)]
    g = rng.integers(-8, 9, size=(B, S, S, C), dtype=np.int8).astype(np.float32)
    return z, np.stack([mean, rstd], axis=1), g


def _window(S, d):
    """window offset d in -1 .. 1 along one axis: (slice of the outputs whose tap is inside the image, slice of those taps)"""
    return slice(max(0, -d), S - max(0, d)), slice(max(0, d), S - max(0, -d))


def _taps(S):
    for code in range(9):
        dy, dx = divmod(code, 3)
        yo, yi = _window(S, dy - 1)
        xo, xi = _window(S, dx - 1)
        yield code, (slice(None), yo, xo), (slice(None), yi, xi)


def max_pool_first(a, want_count=False):
    """3x3 / stride 1 / SAME maximum of a [B,S,S,C] by nine running-maximum passes in window scan order: (max, code of the first
    maximum, and on request how many taps of the window hold the maximum).  Taps outside the image are never looked at."""
    S = a.shape[1]
    best = np.full(a.shape, -np.inf, dtype=a.dtype)
    code = np.zeros(a.shape, dtype=np.uint8)
    for c, o, i in _taps(S):
        bv, cand = best[o], a[i]
        upd = cand > bv                                  # strictly: an equal later tap never replaces an earlier one
        np.copyto(bv, cand, where=upd)
        np.copyto(code[o], np.uint8(c), where=upd)
    count = None
    if want_count:
        count = np.zeros(a.shape, dtype=np.uint8)
        for c, o, i in _taps(S):
            count[o] += a[i] == best[o]
    return best, code, count


def _pool_any(m):
    S = m.shape[1]
    r = np.zeros(m.shape, dtype=bool)
    for c, o, i in _taps(S):
        r[o] |= m[i]
    return r


def pool_backward(code, g):
    """the gradient of every output to the input its code names"""
    S = g.shape[1]
    gin = np.zeros(g.shape, dtype=g.dtype)
    for c, o, i in _taps(S):
        gin[i] += np.where(code[o] == c, g[o], 0)
    return gin


def reference(z, mean_rstd, alpha, g=None, dtype=np.float64, want_count=False):
    """the whole chain in `dtype` (fp64: the reference; fp32: to show that nothing rounds).  Returns a dict:
    xhat, a, out, idx, count (taps holding the maximum; on request), zero_free, and with g: gpool, gxhat, sum_g [C], sum_gx [C]"""
    z = z.astype(dtype)
    mean, rstd = mean_rstd[:, 0].astype(dtype), mean_rstd[:, 1].astype(dtype)
    xhat = (z - mean) * rstd
    a = np.maximum(dtype(alpha) * xhat, xhat)
    out, idx, count = max_pool_first(a, want_count)
    r = {"xhat": xhat, "a": a, "out": out, "idx": idx, "count": count}
    negz = (a == 0) & np.signbit(a)
    zero_free = np.zeros(a.shape, dtype=bool)
    if negz.any():
        any_neg, any_pos = _pool_any(negz), _pool_any((a == 0) & ~np.signbit(a))
        zero = out == 0
        zero_free = zero & any_neg & any_pos
        out[zero & any_pos] = 0.0
        out[zero & any_neg & ~any_pos] = -0.0
    r["zero_free"] = zero_free
    if g is not None:
        gpool = pool_backward(idx, g.astype(dtype))
        gx = np.where(xhat > 0, gpool, gpool * dtype(alpha))
        r.update(gpool=gpool, gxhat=gx, sum_g=gx.sum(axis=(0, 1, 2)), sum_gx=(gx * xhat).sum(axis=(0, 1, 2)))
    return r


def tie_stats(ref):
    """shares of windows that hold a tie for the maximum / a tie at a positive value, and the tie map"""
    tie = ref["count"] >= 2
    return float(tie.mean()), float((tie & (ref["out"] > 0)).mean()), tie


# ------------------------------------------------------------------------------------------------- strip geometry (slide_cfg)
SLIDE_BLOCKS, SLIDE_MINROWS = 5120, 8          # the defaults of the two development switches


def slide_geometry(B, S, C, blocks=SLIDE_BLOCKS, minrows=SLIDE_MINROWS):
    """slide_cfg of pointwise.hip restated: None above 512 channels (the gathering forms), else a dict with TX (image columns per
    workgroup), threads, ncol (column blocks), nstrips, rps (rows per strip), rows (rows of every strip, 0 = empty), empty, and
    workgroups = rows of the backward slab"""
    CQ = C // 4
    if CQ > 128:
        return None
    TX = 256 // CQ
    ncol = -(-S // TX)
    nstrips = 1
    while B * ncol * nstrips < blocks and S // (nstrips * 2) >= minrows:
        nstrips *= 2
    while B * ncol * nstrips < 768 and S // (nstrips * 2) >= 2:
        nstrips *= 2
    rps = -(-S // nstrips)
    rows = [max(0, min(S, (i + 1) * rps) - i * rps) for i in range(nstrips)]
    return {"TX": TX, "threads": TX * CQ, "ncol": ncol, "nstrips": nstrips, "rps": rps, "rows": rows,
            "empty": sum(1 for n in rows if n == 0), "workgroups": B * ncol * nstrips,
            "tiles": ncol * TX == S, "pixels": max(rows) * min(TX, S)}


# The shapes of tests/test_gpu_pool_exact.py: (B, S, C), the two switches (None: the default), alpha, and the geometry the case is
# there for: nstrips, rps, rows of the last non-empty strip, empty strips -- or None for the gathering forms.  test_pool_exact_plan.py
# holds this table to slide_geometry, the GPU test holds slide_geometry to the library.
ONE, DEFAULT = (0, 8), (None, None)            # (0, 8): no workgroup target -> one strip wherever B * ncol >= 768
CASES = [
    # one long strip: 6 turns of the ring of three, and the two ways to leave it early
    ("one_strip_rows_0_mod_3", (384, 18, 64), ONE, 0.25, (1, 18, 18, 0)),
    ("one_strip_rows_1_mod_3", (77, 19, 512), ONE, 0.0, (1, 19, 19, 0)),
    ("one_strip_rows_2_mod_3", (384, 17, 64), ONE, 0.0, (1, 17, 17, 0)),
    ("two_columns_224_threads", (64, 23, 448), ONE, 0.25, (1, 23, 23, 0)),
    ("two_uneven_strips", (384, 17, 64), DEFAULT, 0.25, (2, 9, 8, 0)),
    ("four_strips", (384, 17, 64), (5120, 4), 0.0, (4, 5, 2, 0)),
    ("one_row_strips", (48, 16, 64), (5120, 1), 0.25, (16, 1, 1, 0)),
    ("empty_strips", (12, 33, 128), DEFAULT, 0.0, (16, 3, 3, 5)),
    ("empty_strip_and_one_row_strip", (2, 25, 128), DEFAULT, 0.25, (8, 4, 1, 1)),
    ("more_columns_than_the_patch", (2, 5, 32), DEFAULT, 0.0, (2, 3, 2, 0)),
    ("columns_tile_the_side_two", (1, 6, 512), DEFAULT, 0.25, (2, 3, 3, 0)),
    ("columns_tile_the_side_four", (96, 20, 256), DEFAULT, 0.0, (2, 10, 10, 0)),
    ("side_1", (3, 1, 64), DEFAULT, 0.0, (1, 1, 1, 0)),
    ("side_1_two_columns", (2, 1, 512), DEFAULT, 0.25, (1, 1, 1, 0)),
    ("side_2", (2, 2, 64), DEFAULT, 0.25, (1, 2, 2, 0)),
    ("side_2_two_columns", (3, 2, 448), DEFAULT, 0.0, (1, 2, 2, 0)),
    ("gathering_forms", (1, 5, 576), DEFAULT, 0.25, None),
]
INVARIANCE_SHAPE = (384, 17, 64)
INVARIANCE_SETTINGS = [ONE, DEFAULT, (5120, 4)]          # one strip of 17 rows, 9 + 8, 5 + 5 + 5 + 2


def case_geometry(shape, switches):
    blocks, minrows = switches
    return slide_geometry(*shape, blocks=SLIDE_BLOCKS if blocks is None else blocks, minrows=SLIDE_MINROWS if minrows is None else minrows)


def describe(geo):
    if geo is None:
        return "gathering forms (no strips)"
    live = [n for n in geo["rows"] if n]
    return "TX %d (%d threads) ncol %d nstrips %d rps %d last strip %d empty %d" % (
        geo["TX"], geo["threads"], geo["ncol"], geo["nstrips"], geo["rps"], live[-1], geo["empty"])


def slide_partials(gx, xhat, geo):
    """the slab drs_bn_backward_reduce must leave on the sliding path: row (b * nstrips + strip) * ncol + column block holds the sums
    of its pixels, per channel (sum gx, sum gx * xhat); rows of empty strips are zero.  -> [workgroups, C, 2] fp64"""
    B, S, _, C = gx.shape
    t = gx * xhat
    p = np.zeros((B, geo["nstrips"], geo["ncol"], C, 2))
    for s in range(geo["nstrips"]):
        y0, y1 = s * geo["rps"], min(S, (s + 1) * geo["rps"])
        for k in range(geo["ncol"]):
            x0, x1 = k * geo["TX"], min(S, (k + 1) * geo["TX"])
            if y0 < y1:
                p[:, s, k, :, 0] = gx[:, y0:y1, x0:x1].sum(axis=(1, 2))
                p[:, s, k, :, 1] = t[:, y0:y1, x0:x1].sum(axis=(1, 2))
    return p.reshape(-1, C, 2)
