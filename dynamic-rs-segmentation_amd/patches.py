"""Patch sampling (host) and patch materialisation (device).

Host mirror of /root/reference/isprs_dilated_random.py: `select_batch` :46-58, the patch-size draw
:1727-1737 with `define_multinomial_probs` :61-71, the per-patch augmentation draws inside
`dynamically_create_patches` :288-318 and the sliding-window enumeration of `create_patches_per_map`
:337-400 (beside it, the tile plan of the opt-in overlap-tile inference: `dense_tiles`).  Index work
stays on the host (it is scalar work); every per-pixel operation -- crop,
rotation, noise, flip, normalisation of bands 0..2, zero halo and band padding for conv1 -- happens
in one HIP kernel (drs_crop_normalize) that writes the conv1 input slab directly (and, for the test-time
augmentation of overlap-tile inference, the dihedral symmetries of whole tiles: drs_crop_dihedral, and tiles of
the bilinearly resampled image: drs_crop_resampled; and, for training with scale jitter, the crop that resamples every patch
at a scale of its own: drs_crop_normalize_scaled).

RNG: like the reference, draws come from the global `random` / `numpy.random` streams in the
reference's call order, so seeding both reproduces the reference's sequence.  The one exception is the opt-in scale jitter, whose
draws come from a generator of their own (draw_scales) so that they leave that sequence alone.
"""
import collections
import math
import random

import numpy as np
import torch
from scipy import special

from . import _lib


# ---------------------------------------------------------------------------------------- index sampling
def select_batch(shuffle, batch_size, it, total_size):
    """isprs:46-58: walk the permutation; at its end reshuffle and top up from the new permutation."""
    end = min(it + batch_size, total_size)
    batch = shuffle[it:end]
    if end != total_size:
        return shuffle, batch, it + batch_size
    shuffle = np.asarray(random.sample(range(total_size), total_size))
    short = batch_size - len(batch)
    if short > 0:
        batch = np.concatenate((batch, shuffle[:short]))
    return shuffle, batch, max(short, 0)


def define_multinomial_probs(values, dif_prob=2):
    """isprs:61-71."""
    n = values[-1] - values[0] + 1
    hi = dif_prob * (1.0 / float(n))
    probs = np.full(n, (1.0 - hi * len(values)) / float(n - len(values)))
    probs[np.asarray(values) - values[0]] = hi
    return probs


def draw_patch_size(distribution_type, values, probs=None):
    """isprs:1727-1737 -> (cur_patch_size, cur_size_int)."""
    if distribution_type == "multi_fixed":
        i = np.random.randint(len(values))
        return int(values[i]), i
    if distribution_type == "uniform":
        s = int(np.random.uniform(values[0], values[-1] + 1, 1)[0])
        return s, s - values[0]
    if distribution_type == "multinomial":
        i = int(np.random.multinomial(1, probs).argmax())
        return values[0] + i, i
    if distribution_type == "single_fixed":
        return int(values[0]), None
    raise ValueError("unknown distribution_type " + str(distribution_type))


def window_counts(h, w, crop_size, stride):
    """isprs:344-347."""
    def n(d):
        q, r = divmod(d - crop_size, stride)
        return q + 1 if r == 0 else q + 2
    return n(h), n(w)


def window_start(h, w, crop_size, stride, index, batch_size, flavour="isprs"):
    """flat (row-major) index of the first window of batch `index`.  isprs:353-354 starts batch i at window i*batch_size.
    contest:275-276 divides by the number of window ROWS where the number of columns belongs
    (`offset_h = int(index*batch_size / total_index_h)`), so on a non-square tile its batches start too early (tall tiles:
    windows evaluated twice, the bottom rows never) or too late: reproduced for flavour="contest" because the reference's label
    maps on such tiles are what they are.  coffee:304-309 takes both counts from the height; its tiles are square (500 x 500),
    where all three agree."""
    n_h, n_w = window_counts(h, w, crop_size, stride)
    f = index * batch_size
    if flavour == "contest":
        return (f // n_h) * n_w + f % n_w
    return f


def window_positions(h, w, crop_size, stride, index, batch_size, flavour="isprs"):
    """isprs:337-400 without the pixel copies: (x, y) of the windows of batch `index` (row-major from window_start), the last
    row / column shifted back to end at the border."""
    n_h, n_w = window_counts(h, w, crop_size, stride)
    f0 = window_start(h, w, crop_size, stride, index, batch_size, flavour)
    f = np.arange(f0, max(f0, min(f0 + batch_size, n_h * n_w)))
    x = np.minimum((f // n_w) * stride, h - crop_size)
    y = np.minimum((f % n_w) * stride, w - crop_size)
    return np.stack([x, y], axis=1).astype(np.int64)


def dense_axis(length, T, before, after):
    """One axis of the overlap-tile plan (loops.predict_tile_dense): (origins, core starts, core ends) of the tiles of side T along an
    axis of `length` pixels, for a net whose output pixel p depends on input pixels [p - before, p + after].
    Origins step by T - before - after; the last tile is moved back to end at the border, as windows are (isprs:366-375).  A core
    starts `before` pixels into its tile and ends `after` pixels early, except at an image border, which it reaches; cores are then
    clipped so that they partition [0, length): every pixel belongs to exactly one core, and every core edge that is not an image
    border keeps the margin from its tile's edge.  T = length: one tile."""
    length, T, before, after = int(length), int(T), int(before), int(after)
    if length < 1 or T < 1 or before < 0 or after < 0:
        raise ValueError("dense tiles: length %d, T %d, margins (%d, %d)" % (length, T, before, after))
    if T > length:
        raise ValueError("dense tile side %d exceeds the image side %d" % (T, length))
    if T == length:
        return [0], [0], [length]
    step = T - before - after
    if step < 1:
        raise ValueError("dense tile side %d must exceed the receptive-field margins %d + %d" % (T, before, after))
    n = -(-(length - T) // step) + 1
    origins = [min(i * step, length - T) for i in range(n)]
    starts, ends = [], []
    for i, o in enumerate(origins):
        starts.append(0 if i == 0 else ends[-1])
        ends.append(length if i == n - 1 else o + T - after)
    return origins, starts, ends


def dense_tiles(h, w, T, before, after):
    """The overlap-tile plan of an h x w image: int64 [n][6] rows (y0, x0, cy0, cy1, cx0, cx1) -- tile origin and half-open core box in
    image coordinates -- in row-major tile order, the product of the two axis plans (dense_axis).  Tiles are square: T <= min(h, w)."""
    if int(T) > min(int(h), int(w)):
        raise ValueError("dense tile side %d exceeds min(h, w) = %d (tiles are square)" % (T, min(int(h), int(w))))
    ry, rs, re = dense_axis(h, T, before, after)
    cx, cs, ce = dense_axis(w, T, before, after)
    return np.array([(ry[i], cx[j], rs[i], re[i], cs[j], ce[j]) for i in range(len(ry)) for j in range(len(cx))],
                    dtype=np.int64).reshape(-1, 6)


# ------------------------------------------------------------------- dihedral test-time augmentation (D4)
TTA_GROUPS = {"flip": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def dihedral_apply(x, g, inverse=False):
    """The symmetry g (0..7: bit 0 fx = flip columns, bit 1 fy = flip rows, bit 2 t = transpose; include/drs.h) on the first two axes of
    x, which need not be square: Y = Z[::-1 if fy, ::-1 if fx] with Z = x.swapaxes(0, 1) if t.  inverse=True applies g^-1 (undo the
    flips, then transpose back), which puts a map computed on Y back on x's grid.  Returns a view."""
    g = int(g)
    if not 0 <= g <= 7:
        raise ValueError("dihedral code %r: must be 0..7" % g)
    x = np.asarray(x)
    fy, fx = slice(None, None, -1 if g & 2 else 1), slice(None, None, -1 if g & 1 else 1)
    if inverse:
        x = x[fy, fx]
        return x.swapaxes(0, 1) if g & 4 else x
    z = x.swapaxes(0, 1) if g & 4 else x
    return z[fy, fx]


def dihedral_core_boxes(boxes, T, g):
    """The core boxes of a dense plan (dense_tiles rows (y0, x0, cy0, cy1, cx0, cx1)) as they lie in the g-TRANSFORMED T x T tiles
    (dihedral_apply): rows (0, 0, i0, i1, j0, j1), tile-local and half-open -- position (i, j) of the transformed tile is inside iff
    the tile pixel sigma_g(i, j) it shows is a core pixel.  (A flip mirrors the interval on its axis, the transpose swaps the axes.)"""
    b = np.asarray(boxes, dtype=np.int64)
    r0, r1, c0, c1 = b[:, 2] - b[:, 0], b[:, 3] - b[:, 0], b[:, 4] - b[:, 1], b[:, 5] - b[:, 1]
    if int(g) & 4:
        r0, r1, c0, c1 = c0, c1, r0, r1
    if int(g) & 2:
        r0, r1 = T - r1, T - r0
    if int(g) & 1:
        c0, c1 = T - c1, T - c0
    z = np.zeros_like(r0)
    return np.stack([z, z, r0, r1, c0, c1], axis=1)


def dihedral_index(g, T):
    """The numpy statement of sigma_g and sigma_g^-1 on a T x T tile: ((I, J), (Ii, Ji)), int64 [T][T] each, such that the transformed
    tile is Y = X[I, J] (Y[i][j] = X[sigma_g(i, j)]: flip, then transpose) and logits L of Y land on X's grid as L[Ii, Ji]
    (sigma_g^-1(a, b): transpose, then flip)."""
    T = int(T)
    ii, jj = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    grid = np.stack([ii, jj], axis=-1)
    fwd = np.ascontiguousarray(dihedral_apply(grid, g))
    inv = np.ascontiguousarray(dihedral_apply(grid, g, inverse=True))
    return (fwd[..., 0], fwd[..., 1]), (inv[..., 0], inv[..., 1])


def tta_group(tta):
    """The codes of a test-time augmentation group, ascending: "flip" = (0, 1, 2, 3), "d4" = 0..7, or an explicit tuple / list of
    distinct codes in 0..7 (e.g. (5,)).  Anything else raises ValueError."""
    if isinstance(tta, str):
        if tta not in TTA_GROUPS:
            raise ValueError("test-time augmentation %r: expected one of %s or a tuple of codes 0..7" % (tta, "|".join(TTA_GROUPS)))
        return TTA_GROUPS[tta]
    if not isinstance(tta, (tuple, list)) or not tta:
        raise ValueError("test-time augmentation %r: expected one of %s or a tuple of codes 0..7" % (tta, "|".join(TTA_GROUPS)))
    if not all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) and 0 <= c <= 7 for c in tta) or len(set(tta)) != len(tta):
        raise ValueError("test-time augmentation %r: codes must be distinct integers in 0..7" % (tta,))
    codes = [int(c) for c in tta]
    return tuple(sorted(codes))


# ------------------------------------------------------------------- multi-scale test-time augmentation
SCALE_MIN, SCALE_MAX = 0.25, 4.0


def scaled_size(n, s):
    """The side of an n-pixel axis resampled by the factor s: max(1, floor(n s + 0.5))."""
    return max(1, int(math.floor(int(n) * float(s) + 0.5)))


def check_scales(scales):
    """The scale factors of multi-scale test-time augmentation as a tuple of floats, in the order given (the order of the per-pixel
    sum).  A non-empty list / tuple of distinct finite numbers in [SCALE_MIN, SCALE_MAX]; anything else raises ValueError."""
    if not isinstance(scales, (tuple, list)) or not scales:
        raise ValueError("scales %r: expected a non-empty list of factors in [%g, %g]" % (scales, SCALE_MIN, SCALE_MAX))
    if not all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in scales):
        raise ValueError("scales %r: the factors must be numbers" % (scales,))
    out = tuple(float(v) for v in scales)
    for v in out:
        if not math.isfinite(v) or not SCALE_MIN <= v <= SCALE_MAX:
            raise ValueError("scale %r: must be finite and in [%g, %g]" % (v, SCALE_MIN, SCALE_MAX))
    if len(set(out)) != len(out):
        raise ValueError("scales %r: a factor is given twice" % (scales,))
    return out


# ------------------------------------------------------------------- scale jitter of the training crop
def check_scale_jitter(jitter):
    """The range of the training crop's scale jitter as a pair of floats (lo, hi): two finite numbers lo <= hi inside
    [SCALE_MIN, SCALE_MAX] (a list or tuple; (1, 1) is allowed: every patch at scale 1).  Anything else raises ValueError."""
    form = "expected two numbers lo,hi with %g <= lo <= hi <= %g" % (SCALE_MIN, SCALE_MAX)
    if not isinstance(jitter, (tuple, list)) or len(jitter) != 2:
        raise ValueError("scale jitter %r: %s" % (jitter, form))
    if not all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in jitter):
        raise ValueError("scale jitter %r: %s" % (jitter, form))
    lo, hi = float(jitter[0]), float(jitter[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and SCALE_MIN <= lo <= hi <= SCALE_MAX):
        raise ValueError("scale jitter %r: %s" % (jitter, form))
    return lo, hi


def parse_scale_jitter(text):
    """The value of the command lines' --scale-jitter option: "lo,hi" as check_scale_jitter takes it.  Anything else raises
    ValueError."""
    try:
        vals = [float(t) for t in text.split(",")] if isinstance(text, str) and text and text == text.strip() and " " not in text else None
    except ValueError:
        vals = None
    if vals is None or len(vals) != 2:
        raise ValueError("scale jitter %r: expected lo,hi with %g <= lo <= hi <= %g" % (text, SCALE_MIN, SCALE_MAX))
    return check_scale_jitter(vals)


def jitter_run_seed(seeds):
    """The run seed of the scale draws from the pair loops.sync_rng returns (two 31-bit seeds): one integer below 2^64."""
    return (int(seeds[0]) << 32) | int(seeds[1])


def draw_scales(B, scale_jitter, jitter_key):
    """The scales s_b of the B patches of a GLOBAL batch (float64 [B]), log-uniform on [lo, hi] = scale_jitter: s = exp(ln lo +
    v (ln hi - ln lo)), v uniform in [0, 1), clamped to [lo, hi]; lo == hi gives lo exactly.  The draw comes from a generator of its own,
    np.random.Generator(np.random.Philox(key=jitter_key)) with jitter_key = (run seed, step), two integers in [0, 2^64): it never
    touches `random` or `numpy.random`, so every other draw of a run is what it is without the jitter, and a resumed run (same run
    seed, same step) draws what the uninterrupted run drew."""
    lo, hi = check_scale_jitter(scale_jitter)
    if jitter_key is None or len(jitter_key) != 2 or not all(0 <= int(k) < 2 ** 64 for k in jitter_key):
        raise ValueError("scale jitter: jitter_key %r must be (run seed, step), two integers in [0, 2^64)" % (jitter_key,))
    gen = np.random.Generator(np.random.Philox(key=np.array([int(jitter_key[0]), int(jitter_key[1])], dtype=np.uint64)))
    v = gen.random(int(B))
    llo, lhi = math.log(lo), math.log(hi)
    return np.minimum(np.maximum(np.exp(llo + v * (lhi - llo)), lo), hi)


# ------------------------------------------------------------------- class weights of the training loss
CLASS_WEIGHT_RECIPES = ("balanced", "median")
MAX_CLASSES = 8          # the classifier kernels carry at most eight classes (include/drs.h)


def check_class_weights(w, K):
    """K class weights as the kernels take them: a float32 array [K] of finite, non-negative numbers (a list, tuple or array of exactly
    K numbers; K <= 8).  Anything else raises ValueError."""
    K = int(K)
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError("class weights: %d classes, the kernels carry 1..%d" % (K, MAX_CLASSES))
    if isinstance(w, (str, bytes)) or not isinstance(w, (list, tuple, np.ndarray)):
        raise ValueError("class weights %r: expected %d numbers" % (w, K))
    if not all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in np.asarray(w, dtype=object).reshape(-1)):
        raise ValueError("class weights %r: the weights must be numbers" % (w,))
    a = np.asarray(w, dtype=np.float64).reshape(-1)
    if a.size != K:
        raise ValueError("class weights %r: %d given, the net has %d classes" % (list(a), a.size, K))
    if not np.all(np.isfinite(a)) or np.any(a < 0) or np.any(a > float(np.finfo(np.float32).max)):
        raise ValueError("class weights %r: every weight must be finite and >= 0" % (list(a),))
    return np.ascontiguousarray(a.astype(np.float32))


def class_weights(counts, recipe):
    """The class weights wc [K] (float64) of the weighted training loss from the per-class pixel counts n_k of the training labels
    (TilePool.label_counts).  With N = sum n_k and Kp = the number of classes that occur:
      "balanced": wc_k = N / (Kp n_k), so that sum_k (n_k / N) wc_k = 1: the expected scale of the weighted loss (normalised by the
                  pixel count) is that of the unweighted one;
      "median":   wc_k = median(f) / f_k with f_k = n_k / N, the median over the classes that occur (median-frequency balancing);
      a list / tuple / array of K numbers: taken as given (check_class_weights).
    A class that never occurs gets weight 1: it never enters the sum."""
    n = np.asarray(counts)
    if n.ndim != 1 or not 1 <= n.size <= MAX_CLASSES or not np.issubdtype(n.dtype, np.integer) or np.any(n < 0):
        raise ValueError("class counts %r: expected 1..%d non-negative integers" % (counts, MAX_CLASSES))
    if not isinstance(recipe, str):
        return check_class_weights(recipe, n.size).astype(np.float64)
    if recipe not in CLASS_WEIGHT_RECIPES:
        raise ValueError("class weights %r: expected one of %s or %d numbers" % (recipe, "|".join(CLASS_WEIGHT_RECIPES), n.size))
    w = np.ones(n.size, dtype=np.float64)
    occ = n > 0
    if not occ.any():
        return w
    nk = n[occ].astype(np.float64)
    N = float(nk.sum())
    if recipe == "balanced":
        w[occ] = N / (float(occ.sum()) * nk)
    else:
        f = nk / N
        w[occ] = float(np.median(f)) / f
    return w


def parse_class_weights(text):
    """The value of the command lines' --class-weights option: a recipe name as it stands, or "w0,w1,..." as a tuple of floats (finite,
    >= 0; their count is checked against the net's classes where the net is known).  Anything else raises ValueError."""
    if text in CLASS_WEIGHT_RECIPES:
        return text
    try:
        vals = [float(t) for t in text.split(",")] if text and text == text.strip() and " " not in text else None
    except ValueError:
        vals = None
    if not vals or len(vals) > MAX_CLASSES or not all(math.isfinite(v) and v >= 0 for v in vals):
        raise ValueError("class weights %r: expected %s or up to %d finite weights >= 0 (w0,w1,...)"
                         % (text, "|".join(CLASS_WEIGHT_RECIPES), MAX_CLASSES))
    return tuple(vals)


# ------------------------------------------------------------------- focal loss of the training loss
MAX_FOCAL_GAMMA = 8.0    # the classifier kernels take gamma = 0 (no focal term) or a finite gamma in (0, 8] (include/drs.h)


def check_focal_gamma(g):
    """The focusing parameter of the focal training loss as the kernels take it: a Python float holding a float32 value,
    0 (no focal term: the cross-entropy kernels, bit for bit) or finite in (0, 8].  Negative, NaN, infinite, above 8 or not a number:
    ValueError."""
    if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, float, np.integer, np.floating)):
        raise ValueError("focal gamma %r: expected a number, 0 or in (0, %g]" % (g, MAX_FOCAL_GAMMA))
    v = float(g)
    if not math.isfinite(v) or v < 0.0 or v > MAX_FOCAL_GAMMA:
        raise ValueError("focal gamma %r: expected 0 or a finite value in (0, %g]" % (g, MAX_FOCAL_GAMMA))
    return float(np.float32(v))


def parse_focal_gamma(text):
    """The value of the command lines' --focal-gamma option: one number as check_focal_gamma takes it.  Anything else raises
    ValueError."""
    try:
        v = float(text) if text and text == text.strip() else None
    except ValueError:
        v = None
    if v is None:
        raise ValueError("focal gamma %r: expected one number, 0 or in (0, %g]" % (text, MAX_FOCAL_GAMMA))
    return check_focal_gamma(v)


# ------------------------------------------------------------------- boundary weight of the training loss
MAX_BOUNDARY_A, MAX_BOUNDARY_SIGMA, MAX_BOUNDARY_R = 64.0, 64.0, 16    # the ranges drs_net_set_boundary_weight takes (include/drs.h)
DEFAULT_BOUNDARY_SIGMA = 4.0


def default_boundary_radius(sigma):
    """the window radius when none is given: three sigma, at most the 16 the kernel's LDS halo holds"""
    return min(MAX_BOUNDARY_R, max(1, int(math.ceil(3.0 * sigma))))


def check_boundary_weight(bw):
    """The boundary weight of the training loss as the library takes it: (a, sigma, R) -- or (a,), (a, sigma), or a
    bare number a -- with a finite in [-1, 64] (0: off), sigma finite in (0, 64] (default 4) and R an integer in 1..16 (default
    min(16, ceil(3 sigma))).  Returns the triple (float, float, int).  Anything else: ValueError."""
    t = tuple(bw) if isinstance(bw, (tuple, list)) else (bw,)
    what = "boundary weight %r: expected a[, sigma[, R]] with a in [-1, %g], sigma in (0, %g], R an integer in 1..%d" % (
        bw, MAX_BOUNDARY_A, MAX_BOUNDARY_SIGMA, MAX_BOUNDARY_R)
    if not 1 <= len(t) <= 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) for v in t):
        raise ValueError(what)
    a = float(t[0])
    sigma = float(t[1]) if len(t) > 1 else DEFAULT_BOUNDARY_SIGMA
    if not math.isfinite(a) or a < -1.0 or a > MAX_BOUNDARY_A or not math.isfinite(sigma) or not 0.0 < sigma <= MAX_BOUNDARY_SIGMA:
        raise ValueError(what)
    if len(t) > 2:
        if not isinstance(t[2], (int, np.integer)) and float(t[2]) != int(t[2]):
            raise ValueError(what)
        radius = int(t[2])
    else:
        radius = default_boundary_radius(sigma)
    if not 1 <= radius <= MAX_BOUNDARY_R:
        raise ValueError(what)
    return a, sigma, radius


def parse_boundary_weight(text):
    """The value of the command lines' --boundary-weight option: `a`, `a,sigma` or `a,sigma,R` as check_boundary_weight takes them (R
    written as an integer).  Anything else raises ValueError."""
    vals = None
    if text and text == text.strip():
        parts = text.split(",")
        try:
            if 1 <= len(parts) <= 3 and all(q and q == q.strip() for q in parts):
                vals = [float(q) for q in parts[:2]] + [int(q) for q in parts[2:]]
        except ValueError:
            vals = None
    if vals is None:
        raise ValueError("boundary weight %r: expected a[,sigma[,R]] (numbers; R an integer)" % (text,))
    return check_boundary_weight(tuple(vals))


# ------------------------------------------------------------------- soft Dice / Tversky term of the training loss
MAX_DICE_LAMBDA, MAX_DICE_SMOOTH = 64.0, float(1 << 20)     # the ranges drs_net_set_dice takes (include/drs.h)
DEFAULT_DICE = (0.0, 0.5, 0.5, 1.0)                         # off; alpha = beta = 0.5 is the Dice score, smooth = 1


def check_dice(dice):
    """The soft Dice / Tversky term of the training loss as the library takes it: (lam, alpha, beta, smooth) -- or
    (lam,), (lam, alpha, beta), or a bare number lam -- with lam finite in [0, 64] (0: off), alpha and beta in [0, 1] (default 0.5
    each: Dice; they come as a pair) and smooth finite in (0, 2^20] (default 1).  Returns the quadruple of floats.  Anything else:
    ValueError."""
    t = tuple(dice) if isinstance(dice, (tuple, list)) else (dice,)
    what = "dice weight %r: expected lam[, alpha, beta[, smooth]] with lam in [0, %g], alpha and beta in [0, 1], smooth in (0, %g]" % (
        dice, MAX_DICE_LAMBDA, MAX_DICE_SMOOTH)
    if len(t) not in (1, 3, 4) or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) for v in t):
        raise ValueError(what)
    v = [float(x) for x in t] + list(DEFAULT_DICE[1:3] if len(t) == 1 else ()) + list(DEFAULT_DICE[3:] if len(t) < 4 else ())
    lam, alpha, beta, smooth = v
    if not math.isfinite(lam) or lam < 0.0 or lam > MAX_DICE_LAMBDA or not 0.0 <= alpha <= 1.0 or not 0.0 <= beta <= 1.0:
        raise ValueError(what)
    if not math.isfinite(smooth) or not 0.0 < smooth <= MAX_DICE_SMOOTH:
        raise ValueError(what)
    return lam, alpha, beta, smooth


def parse_dice(text):
    """The value of the command lines' --dice-weight option: `lam`, `lam,alpha,beta` or `lam,alpha,beta,smooth` as check_dice takes
    them.  Anything else raises ValueError."""
    vals = None
    if text and text == text.strip():
        parts = text.split(",")
        try:
            if len(parts) in (1, 3, 4) and all(q and q == q.strip() for q in parts):
                vals = [float(q) for q in parts]
        except ValueError:
            vals = None
    if vals is None:
        raise ValueError("dice weight %r: expected lam[,alpha,beta[,smooth]] (numbers)" % (text,))
    return check_dice(tuple(vals))


# ------------------------------------------------------------------- hard example mining in the training loss
MAX_HARD_MIN_KEEP = (1 << 24) - 1      # the range drs_net_set_hard_mining takes (include/drs.h)
DEFAULT_HARD_MINING = (1.0, 0)         # off: every pixel in the loss is kept


def check_hard_mining(hard_mining):
    """Online hard example mining in the training loss as the library takes it: (keep, min_keep) -- or (keep,), or a
    bare number keep -- with keep finite in (0, 1] (1: off) and min_keep an integer in [0, 2^24) (default 0).  Returns (float, int).
    Anything else: ValueError."""
    t = tuple(hard_mining) if isinstance(hard_mining, (tuple, list)) else (hard_mining,)
    what = "hard mining %r: expected keep[, min_keep] with keep in (0, 1] and min_keep an integer in [0, %d]" % (hard_mining, MAX_HARD_MIN_KEEP)
    if len(t) not in (1, 2) or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) for v in t):
        raise ValueError(what)
    keep = float(t[0])
    min_keep = t[1] if len(t) == 2 else DEFAULT_HARD_MINING[1]
    if not math.isfinite(keep) or not 0.0 < keep <= 1.0:
        raise ValueError(what)
    if isinstance(min_keep, (float, np.floating)):
        if not math.isfinite(min_keep) or min_keep != int(min_keep):
            raise ValueError(what)
    min_keep = int(min_keep)
    if not 0 <= min_keep <= MAX_HARD_MIN_KEEP:
        raise ValueError(what)
    return keep, min_keep


def parse_hard_mining(text):
    """The value of the command lines' --hard-mining option: `keep` or `keep,min_keep` as check_hard_mining takes them (min_keep in
    decimal digits).  Anything else raises ValueError."""
    vals = None
    if text and text == text.strip():
        parts = text.split(",")
        try:
            if len(parts) in (1, 2) and all(q and q == q.strip() for q in parts) and (len(parts) == 1 or parts[1].isdigit()):
                vals = [float(parts[0])] + [int(q) for q in parts[1:]]
        except ValueError:
            vals = None
    if vals is None:
        raise ValueError("hard mining %r: expected keep[,min_keep] (a number and an integer)" % (text,))
    return check_hard_mining(tuple(vals))


# ------------------------------------------------------------------- Lovasz-softmax term of the training loss
MAX_LOVASZ_LAMBDA = 64.0               # the range drs_net_set_lovasz takes (include/drs.h)
DEFAULT_LOVASZ = 0.0                   # off


def check_lovasz(lovasz):
    """The Lovasz-softmax term of the training loss as the library takes it: a number lam -- or (lam,) -- finite in
    [0, 64] (0: off).  Returns the float.  Anything else: ValueError."""
    t = tuple(lovasz) if isinstance(lovasz, (tuple, list)) else (lovasz,)
    what = "lovasz weight %r: expected lam in [0, %g]" % (lovasz, MAX_LOVASZ_LAMBDA)
    if len(t) != 1 or isinstance(t[0], (bool, np.bool_)) or not isinstance(t[0], (int, float, np.integer, np.floating)):
        raise ValueError(what)
    lam = float(t[0])
    if not math.isfinite(lam) or lam < 0.0 or lam > MAX_LOVASZ_LAMBDA:
        raise ValueError(what)
    return lam


def parse_lovasz(text):
    """The value of the command lines' --lovasz-weight option: `lam` as check_lovasz takes it.  Anything else raises ValueError."""
    val = None
    if text and text == text.strip() and "," not in text:
        try:
            val = float(text)
        except ValueError:
            val = None
    if val is None:
        raise ValueError("lovasz weight %r: expected lam (a number)" % (text,))
    return check_lovasz(val)


# ------------------------------------------------------------------- boundary (surface) loss of the training loss
MAX_SURFACE_LAMBDA = 64.0              # the ranges drs_net_set_surface_loss takes (include/drs.h)
MAX_SURFACE_CLIP = 32768.0
DEFAULT_SURFACE_LOSS = (0.0, 0.0)      # off; clip 0: the distances are not clipped


def check_surface_loss(surface_loss):
    """The boundary (surface) loss of the training loss as the library takes it: (lam, clip) -- or (lam,), or a bare
    number lam -- with lam finite in [0, 64] (0: off) and clip 0 (none, the default) or finite in [1, 32768] pixels.  Returns
    (float, float).  Anything else: ValueError."""
    t = tuple(surface_loss) if isinstance(surface_loss, (tuple, list)) else (surface_loss,)
    what = "surface loss %r: expected lam[, clip] with lam in [0, %g] and clip 0 or in [1, %g]" % (surface_loss, MAX_SURFACE_LAMBDA,
                                                                                                 MAX_SURFACE_CLIP)
    if len(t) not in (1, 2) or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) for v in t):
        raise ValueError(what)
    lam = float(t[0])
    clip = float(t[1]) if len(t) == 2 else DEFAULT_SURFACE_LOSS[1]
    if not math.isfinite(lam) or lam < 0.0 or lam > MAX_SURFACE_LAMBDA:
        raise ValueError(what)
    if not math.isfinite(clip) or not (clip == 0.0 or 1.0 <= clip <= MAX_SURFACE_CLIP):
        raise ValueError(what)
    return lam, clip + 0.0


def parse_surface_loss(text):
    """The value of the command lines' --surface-loss option: `lam` or `lam,clip` as check_surface_loss takes them.  Anything else
    raises ValueError."""
    vals = None
    if text and text == text.strip():
        parts = text.split(",")
        try:
            if len(parts) in (1, 2) and all(q and q == q.strip() for q in parts):
                vals = [float(q) for q in parts]
        except ValueError:
            vals = None
    if vals is None:
        raise ValueError("surface loss %r: expected lam[,clip] (numbers)" % (text,))
    return check_surface_loss(tuple(vals))


# ------------------------------------------------------------------- per-pixel score maps of whole-tile inference
SCORE_KINDS = ("confidence", "margin", "entropy")     # the uint8 maps of drs_stitch_finalize_scores


def check_score_kinds(kinds):
    """The score maps asked of an inference path as a tuple of names in the order given: a non-empty tuple / list of distinct names
    from SCORE_KINDS.  Anything else raises ValueError."""
    if isinstance(kinds, (str, bytes)) or not isinstance(kinds, (tuple, list)) or not kinds:
        raise ValueError("score maps %r: expected a non-empty tuple of names from %s" % (kinds, "|".join(SCORE_KINDS)))
    for k in kinds:
        if k not in SCORE_KINDS:
            raise ValueError("score map %r: expected one of %s" % (k, "|".join(SCORE_KINDS)))
    if len(set(kinds)) != len(kinds):
        raise ValueError("score maps %r: a name is given twice" % (tuple(kinds),))
    return tuple(kinds)


def parse_score_maps(text):
    """The value of the command line's --score-maps option: "confidence,entropy" as a tuple of names (check_score_kinds).  An empty
    value, blanks, an unknown or a repeated name raise ValueError."""
    names = text.split(",") if isinstance(text, str) and text and text == text.strip() and " " not in text else None
    if not names or any(n not in SCORE_KINDS for n in names) or len(set(names)) != len(names):
        raise ValueError("score maps %r: expected distinct names from %s, comma-separated (e.g. confidence,entropy)"
                         % (text, "|".join(SCORE_KINDS)))
    return tuple(names)


# ------------------------------------------------------------------- temperature scaling of the score maps
BETA_MIN, BETA_MAX = 1.0 / 64.0, 64.0     # the inverse temperatures include/drs.h accepts


def check_temperature_beta(beta):
    """An inverse temperature beta = 1 / T as the float the kernels take (rounded to float32): a finite number in [1/64, 64].
    Anything else raises ValueError."""
    try:
        ok = not isinstance(beta, (bool, str, bytes)) and math.isfinite(float(beta))
    except (TypeError, ValueError):
        ok = False
    b = float(np.float32(beta)) if ok else 0.0
    if not BETA_MIN <= b <= BETA_MAX:
        raise ValueError("temperature beta %r: expected a finite inverse temperature in [1/64, 64]" % (beta,))
    return b


def parse_temperature(text):
    """The value of the command line's --temperature option: "auto" (the fitted file of the step being evaluated), or a temperature
    T > 0 whose inverse is an accepted beta, returned as beta = 1 / T (check_temperature_beta).  Anything else raises ValueError."""
    if text == "auto":
        return "auto"
    try:
        ok = isinstance(text, str) and text == text.strip() and text != ""
        T = float(text) if ok else 0.0
    except ValueError:
        T = 0.0
    if not (math.isfinite(T) and T > 0.0):
        raise ValueError("temperature %r: expected auto or a temperature T > 0 with 1/64 <= 1/T <= 64" % (text,))
    try:
        return check_temperature_beta(1.0 / T)
    except ValueError:
        raise ValueError("temperature %r: expected auto or a temperature T > 0 with 1/64 <= 1/T <= 64" % (text,)) from None


# ------------------------------------------------------------------- local dense-CRF refinement of whole maps
CrfParams = collections.namedtuple("CrfParams", "iters radius step w_app theta_xy theta_rgb w_smooth theta_s")
CRF_DEFAULTS = CrfParams(5, 5, 2, 4.0, 8.0, 0.08, 2.0, 2.0)
CRF_MAX_ITERS, CRF_MAX_RADIUS, CRF_MAX_STEP, CRF_MAX_REACH = 10, 6, 4, 12     # the ranges include/drs.h accepts (iterations: the host's)
CRF_FORM = ("iters in 1..%d, radius in 1..%d, step in 1..%d with radius * step <= %d, w_app >= 0, theta_xy > 0, theta_rgb > 0, "
            "w_smooth >= 0, theta_s > 0" % (CRF_MAX_ITERS, CRF_MAX_RADIUS, CRF_MAX_STEP, CRF_MAX_REACH))


def check_crf(spec):
    """The `crf` option of validate_test / generate_final_maps as a CrfParams: True or "crf" (the defaults), an int (the iterations,
    everything else at its default), a dict of some of CrfParams' fields, or all eight as a tuple / list in CrfParams' order.  The
    thetas of position are in pixels, theta_rgb in the units of the tiles' values.  Anything else, or a value outside its range,
    raises ValueError naming the ranges."""
    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)

    def is_num(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(float(v))
    if spec is True or (isinstance(spec, str) and spec == "crf"):
        p = CRF_DEFAULTS
    elif is_int(spec):
        p = CRF_DEFAULTS._replace(iters=int(spec))
    elif isinstance(spec, dict):
        unknown = [k for k in spec if k not in CrfParams._fields]
        if unknown:
            raise ValueError("crf %r: unknown parameter %r; expected some of %s" % (spec, unknown[0], ", ".join(CrfParams._fields)))
        p = CRF_DEFAULTS._replace(**spec)
    elif isinstance(spec, (tuple, list)) and len(spec) == len(CrfParams._fields):
        p = CrfParams(*spec)
    else:
        raise ValueError("crf %r: expected True, \"crf\", the iterations, a dict or the 8 values (%s): %s"
                         % (spec, ", ".join(CrfParams._fields), CRF_FORM))
    if not all(is_int(v) for v in p[:3]) or not all(is_num(v) for v in p[3:]):
        raise ValueError("crf %r: iters, radius and step are integers, the rest finite numbers: %s" % (spec, CRF_FORM))
    p = CrfParams(int(p.iters), int(p.radius), int(p.step), *[float(v) for v in p[3:]])
    ok = (1 <= p.iters <= CRF_MAX_ITERS and 1 <= p.radius <= CRF_MAX_RADIUS and 1 <= p.step <= CRF_MAX_STEP
          and p.radius * p.step <= CRF_MAX_REACH and p.w_app >= 0 and p.w_smooth >= 0
          and all(np.float32(t) > 0 for t in (p.theta_xy, p.theta_rgb, p.theta_s)))
    if not ok:
        raise ValueError("crf %r: out of range: %s" % (spec, CRF_FORM))
    return p


def parse_crf_iters(text):
    """The value of the command line's --crf=ITERS: the iterations as an int in 1..10.  Anything else raises ValueError."""
    if not (isinstance(text, str) and text.isascii() and text.isdigit()) or not 1 <= int(text) <= CRF_MAX_ITERS:
        raise ValueError("crf iterations %r: expected an integer in 1..%d" % (text, CRF_MAX_ITERS))
    return int(text)


def parse_crf_params(text):
    """The value of the command line's --crf-params: "R,step,w_app,theta_xy,theta_rgb,w_smooth,theta_s" as the dict check_crf takes
    (the iterations are --crf's).  Anything else raises ValueError."""
    names = CrfParams._fields[1:]
    parts = text.split(",") if isinstance(text, str) and text and text == text.strip() and " " not in text else []
    try:
        if len(parts) != len(names) or not all(t.isascii() and t.isdigit() for t in parts[:2]):
            raise ValueError(text)
        spec = dict(zip(names, [int(parts[0]), int(parts[1])] + [float(t) for t in parts[2:]]))
        check_crf(spec)
    except ValueError:
        raise ValueError("crf parameters %r: expected %s with %s" % (text, ",".join(names), CRF_FORM)) from None
    return spec


# ------------------------------------------------------------------- boundary-quality scores of validation
BOUNDARY_DEFAULT = (1, 2, 4, 8)
BOUNDARY_MAX_DISTANCES, BOUNDARY_MAX_REACH = 8, 16     # the ranges include/drs.h accepts


def check_boundary_distances(v):
    """The band distances of the boundary scores, in pixels, as a tuple of ints: 1 to 8 integers in 1..16, strictly ascending
    (drs_boundary_histogram's).  Anything else raises ValueError naming the offending value."""
    form = "1 to %d integers in 1..%d, strictly ascending" % (BOUNDARY_MAX_DISTANCES, BOUNDARY_MAX_REACH)
    if isinstance(v, (str, bytes)) or not isinstance(v, (tuple, list, np.ndarray)) or not 1 <= len(v) <= BOUNDARY_MAX_DISTANCES:
        raise ValueError("boundary distances %r: expected %s" % (v, form))
    out = []
    for d in v:
        if not isinstance(d, (int, np.integer)) or isinstance(d, bool) or not 1 <= int(d) <= BOUNDARY_MAX_REACH:
            raise ValueError("boundary distance %r of %r: expected %s" % (d, tuple(v), form))
        if out and int(d) <= out[-1]:
            raise ValueError("boundary distance %r of %r does not exceed the one before it: expected %s" % (d, tuple(v), form))
        out.append(int(d))
    return tuple(out)


def parse_boundary_scores(text):
    """The value of the command line's --boundary-scores option: "1,2,4,8" as a tuple of ints (check_boundary_distances).  An empty
    value, blanks, or anything that is not a plain decimal integer raise ValueError."""
    parts = text.split(",") if isinstance(text, str) and text and text == text.strip() and " " not in text else []
    for t in parts:
        if not (t.isascii() and t.isdigit()):
            raise ValueError("boundary distance %r of %r: expected integers, comma-separated (e.g. 1,2,4,8)" % (t, text))
    if not parts:
        raise ValueError("boundary distances %r: expected integers, comma-separated (e.g. 1,2,4,8)" % (text,))
    return check_boundary_distances([int(t) for t in parts])


# ------------------------------------------------------------------- sieve of whole-map labels: a minimum mapping unit
SIEVE_MAX_ROUNDS = 64
SIEVE_CONNECTIVITY = 4                     # gdal_sieve's default
SIEVE_MAX_CLASSES, SIEVE_MAX_SIZE = 32, 1 << 30        # the ranges include/drs.h accepts
SieveParams = collections.namedtuple("SieveParams", "min_size connectivity")


def _sieve_size(v, of):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) <= SIEVE_MAX_SIZE:
        raise ValueError("sieve threshold %r%s: expected an integer in 0..2^30 (pixels)" % (v, of))
    return int(v)


def check_sieve(spec):
    """The sieve's parameters as SieveParams(min_size, connectivity).  spec: an int (one threshold in pixels for every class), a
    sequence of 1 to 32 ints (one per class; loops.sieve_labels wants exactly K or one), a dict {"min_size": either of those,
    "connectivity": 4 | 8} (connectivity optional), or a SieveParams.  min_size comes back as a tuple of ints in 0..2^30 -- of ONE
    int for a scalar spec: it stands for every class --, connectivity as 4 (the default, gdal_sieve's) or 8.  Anything else raises
    ValueError naming the offending value."""
    connectivity = SIEVE_CONNECTIVITY
    if isinstance(spec, SieveParams):
        spec = spec._asdict()
    if isinstance(spec, dict):
        unknown = sorted(set(spec) - {"min_size", "connectivity"})
        if unknown or "min_size" not in spec:
            raise ValueError("sieve %r: expected the keys min_size and, optionally, connectivity%s"
                             % (spec, "; unknown: " + ", ".join(map(repr, unknown)) if unknown else ""))
        connectivity = spec.get("connectivity", SIEVE_CONNECTIVITY)
        if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
            raise ValueError("sieve connectivity %r: expected 4 or 8" % (connectivity,))
        spec = spec["min_size"]
    if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
        return SieveParams((_sieve_size(spec, ""),), int(connectivity))
    if isinstance(spec, (str, bytes)) or not isinstance(spec, (tuple, list, np.ndarray)) or not 1 <= len(spec) <= SIEVE_MAX_CLASSES:
        raise ValueError("sieve thresholds %r: expected an integer or 1 to %d integers in 0..2^30, one per class" % (spec, SIEVE_MAX_CLASSES))
    return SieveParams(tuple(_sieve_size(v, " of %r" % (tuple(spec),)) for v in spec), int(connectivity))


def sieve_thresholds(sieve, K):
    """the K thresholds of a SieveParams for a net of K classes; a count other than 1 or K raises ValueError"""
    if not 1 <= K <= SIEVE_MAX_CLASSES:
        raise ValueError("sieve: %r classes, expected 1..%d" % (K, SIEVE_MAX_CLASSES))
    if len(sieve.min_size) == 1:
        return sieve.min_size * K
    if len(sieve.min_size) != K:
        raise ValueError("sieve thresholds %r: %d given, expected 1 or %d (one per class)" % (sieve.min_size, len(sieve.min_size), K))
    return sieve.min_size


def parse_sieve(text):
    """The value of the command line's --sieve option: "N" or "n0,n1,..." as check_sieve's min_size (a tuple of ints).  An empty
    value, blanks, or anything that is not a plain decimal integer raise ValueError."""
    parts = text.split(",") if isinstance(text, str) and text and text == text.strip() and " " not in text else []
    for t in parts:
        if not (t.isascii() and t.isdigit()):
            raise ValueError("sieve threshold %r of %r: expected integers, comma-separated (e.g. 16 or 32,32,8,32,4,0)" % (t, text))
    if not parts:
        raise ValueError("sieve thresholds %r: expected integers, comma-separated (e.g. 16 or 32,32,8,32,4,0)" % (text,))
    return check_sieve([int(t) for t in parts]).min_size


# ------------------------------------------------------------------- superpixel vote of whole-map labels
SUPERPIXEL_WEIGHTS = ("labels", "confidence")
SUPERPIXEL_RANGES = (("size", 4, 32), ("compactness", 1, 40), ("iters", 1, 16))        # the ranges include/drs.h accepts
SuperpixelParams = collections.namedtuple("SuperpixelParams", "size compactness iters weight")
SUPERPIXEL_DEFAULTS = SuperpixelParams(8, 10, 5, "labels")


def check_superpixel(spec):
    """The superpixel vote's parameters as SuperpixelParams(size, compactness, iters, weight).  spec: None or True (the defaults:
    size 8, compactness 10, iters 5, weight "labels"), an int (the size: the grid step in pixels), a sequence of 1 to 3 ints (size,
    compactness, iters), a dict with any of the four keys, or a SuperpixelParams.  size in 4..32, compactness in 1..40, iters in
    1..16, weight "labels" (every pixel votes once) or "confidence" (a pixel votes with its confidence byte).  Anything else raises
    ValueError naming the offending value."""
    if spec is None or spec is True:
        return SUPERPIXEL_DEFAULTS
    if isinstance(spec, SuperpixelParams):
        spec = spec._asdict()
    elif isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
        spec = {"size": spec}
    elif isinstance(spec, (tuple, list, np.ndarray)) and not isinstance(spec, (str, bytes)):
        if not 1 <= len(spec) <= 3:
            raise ValueError("superpixel %r: expected 1 to 3 integers: size, compactness, iters" % (tuple(spec),))
        spec = dict(zip(("size", "compactness", "iters"), spec))
    if not isinstance(spec, dict):
        raise ValueError("superpixel %r: expected a size, (size, compactness, iters), or a dict with the keys %s"
                         % (spec, ", ".join(SuperpixelParams._fields)))
    unknown = sorted(set(spec) - set(SuperpixelParams._fields))
    if unknown:
        raise ValueError("superpixel %r: expected the keys %s; unknown: %s"
                         % (spec, ", ".join(SuperpixelParams._fields), ", ".join(map(repr, unknown))))
    out = SUPERPIXEL_DEFAULTS._asdict()
    for name, lo, hi in SUPERPIXEL_RANGES:
        v = spec.get(name, out[name])
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= int(v) <= hi:
            raise ValueError("superpixel %s %r: expected an integer in %d..%d" % (name, v, lo, hi))
        out[name] = int(v)
    weight = spec.get("weight", out["weight"])
    if not isinstance(weight, str) or weight not in SUPERPIXEL_WEIGHTS:
        raise ValueError("superpixel weight %r: expected %s" % (weight, " or ".join(SUPERPIXEL_WEIGHTS)))
    return SuperpixelParams(out["size"], out["compactness"], out["iters"], weight)


def parse_superpixel(text):
    """The value of the command line's --superpixel-vote option: "size", "size,compactness" or "size,compactness,iters" as a tuple of
    ints within check_superpixel's ranges.  An empty value, blanks, or anything that is not a plain decimal integer raise ValueError."""
    form = "expected size[,compactness[,iters]] as integers, comma-separated (e.g. 8 or 8,10,5)"
    parts = text.split(",") if isinstance(text, str) and text and text == text.strip() and " " not in text else []
    for t in parts:
        if not (t.isascii() and t.isdigit()):
            raise ValueError("superpixel value %r of %r: %s" % (t, text, form))
    if not 1 <= len(parts) <= 3:
        raise ValueError("superpixel values %r: %s" % (text, form))
    return tuple(check_superpixel([int(t) for t in parts])[:len(parts)])


# ------------------------------------------------------------------- polygon output of whole-map labels
POLYGON_CONNECTIVITY = 4                   # what holds a polygon together by default: the sieve's default


def check_polygons(v):
    """The connectivity of the polygon output as an int: 4 (the default) or 8 (drs_components').  Anything else raises ValueError
    naming the offending value."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in (4, 8):
        raise ValueError("polygons connectivity %r: expected 4 or 8" % (v,))
    return int(v)


def parse_polygons(text):
    """The value of the command line's --polygons option: "4" or "8" as an int (check_polygons).  Anything else raises ValueError."""
    if not isinstance(text, str) or text not in ("4", "8"):
        raise ValueError("polygons connectivity %r: expected 4 or 8" % (text,))
    return check_polygons(int(text))


# ------------------------------------------------------------------- object-level scores of validation
OBJECT_CONNECTIVITY = 4                    # what holds an object together by default: the sieve's default


def check_object_scores(v):
    """The connectivity of the object scores as an int: 4 (the default) or 8 (drs_components').  Anything else raises ValueError
    naming the offending value."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in (4, 8):
        raise ValueError("object scores connectivity %r: expected 4 or 8" % (v,))
    return int(v)


def parse_object_scores(text):
    """The value of the command line's --object-scores option: "4" or "8" as an int (check_object_scores).  Anything else raises
    ValueError."""
    if not isinstance(text, str) or text not in ("4", "8"):
        raise ValueError("object scores connectivity %r: expected 4 or 8" % (text,))
    return check_object_scores(int(text))


# ------------------------------------------------------------------- surface-distance scores of validation
SURFACE_DEFAULT = (1, 2, 4, 8)
SURFACE_MAX_TOLERANCES, SURFACE_MAX_TOLERANCE = 8, 255


def check_surface_tolerances(v):
    """The tolerances of the normalised surface Dice, in pixels, as a tuple of ints: 1 to 8 integers in 1..255, strictly ascending.
    Anything else raises ValueError naming the offending value."""
    form = "1 to %d integers in 1..%d, strictly ascending" % (SURFACE_MAX_TOLERANCES, SURFACE_MAX_TOLERANCE)
    if isinstance(v, (str, bytes)) or not isinstance(v, (tuple, list, np.ndarray)) or not 1 <= len(v) <= SURFACE_MAX_TOLERANCES:
        raise ValueError("surface tolerances %r: expected %s" % (v, form))
    out = []
    for d in v:
        if not isinstance(d, (int, np.integer)) or isinstance(d, bool) or not 1 <= int(d) <= SURFACE_MAX_TOLERANCE:
            raise ValueError("surface tolerance %r of %r: expected %s" % (d, tuple(v), form))
        if out and int(d) <= out[-1]:
            raise ValueError("surface tolerance %r of %r does not exceed the one before it: expected %s" % (d, tuple(v), form))
        out.append(int(d))
    return tuple(out)


def parse_surface_scores(text):
    """The value of the command line's --surface-scores option: "1,2,4,8" as a tuple of ints (check_surface_tolerances).  An empty
    value, blanks, or anything that is not a plain decimal integer raise ValueError."""
    parts = text.split(",") if isinstance(text, str) and text and text == text.strip() and " " not in text else []
    for t in parts:
        if not (t.isascii() and t.isdigit()):
            raise ValueError("surface tolerance %r of %r: expected integers, comma-separated (e.g. 1,2,4,8)" % (t, text))
    if not parts:
        raise ValueError("surface tolerances %r: expected integers, comma-separated (e.g. 1,2,4,8)" % (text,))
    return check_surface_tolerances([int(t) for t in parts])


# ---------------------------------------------------------------------------------------- augmentation draws
def rotation_params(angle_deg, S):
    """(m00, m01, m10, m11, off0, off1) that scipy.ndimage.rotate(reshape=False) hands to its
    geometric transform for an S x S plane (output -> input coordinates)."""
    c, s = special.cosdg(angle_deg), special.sindg(angle_deg)
    m = np.array([[c, s], [-s, c]])
    centre = (np.array([S, S]) - 1) / 2
    off = centre - m @ centre
    return np.array([m[0, 0], m[0, 1], m[1, 0], m[1, 1], off[0], off[1]], dtype=np.float64)


def nearest_source_index(params, S):
    """numpy statement of what the kernel evaluates per output pixel: order-0 geometric transform of
    ndimage (in = M.out + off accumulated left to right, nearest = floor(c + 0.5), zero fill outside
    [0, S-1]).  Returns (src_row, src_col, valid) arrays [S, S]."""
    i, j = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    c0 = ((0.0 + i * params[0]) + j * params[1]) + params[4]
    c1 = ((0.0 + i * params[2]) + j * params[3]) + params[5]
    valid = ~((c0 < 0) | (c0 > S - 1) | (c1 < 0) | (c1 > S - 1))
    return np.floor(c0 + 0.5).astype(np.int64), np.floor(c1 + 0.5).astype(np.int64), valid


class Augmentation(object):
    """Per-batch augmentation decisions, drawn in the reference's order (isprs:288-318)."""

    def __init__(self, B):
        self.rot_on = np.zeros(B, dtype=np.uint8)
        self.rot = np.zeros((B, 6), dtype=np.float64)
        self.noise_on = np.zeros(B, dtype=np.uint8)
        self.flip = np.zeros(B, dtype=np.int32)
        self.noise = None          # [B, S, S, C] float64 when host noise is used
        self.seed = 0
        self.index0 = 0            # place of the first patch in the global batch (device noise is keyed by the global index)
        self.scale = None          # [B] float64: the scale of every patch when the crop jitters the scale (draw_scales)
        self.geo = None            # [B, 3] float64 (step, cy, cx): the footprints of those patches (scale_geometry); set = the scaled crop

    def shard(self, sl):
        """this rank's slice `sl` of a global batch's draws (every per-patch table; the noise seed stays, index0 = sl.start: device
        noise is keyed by the patch's place in the global batch)"""
        mine = Augmentation(len(self.flip[sl]))
        mine.rot_on, mine.rot, mine.noise_on, mine.flip = self.rot_on[sl], self.rot[sl], self.noise_on[sl], self.flip[sl]
        mine.noise = self.noise[sl] if self.noise is not None else None
        mine.scale = self.scale[sl] if self.scale is not None else None
        mine.seed, mine.index0 = self.seed, sl.start
        return mine


def draw_augmentation(instances, S, C, noise="device", scale_jitter=None, jitter_key=None):
    """For every instance, in order: randint(0,2) rotate?; randint(0,2) noise? [+ normal(0, .01, (S,S,C))
    when noise == 'host': bit-exact with the reference]; randint(0,3) flip.
    scale_jitter = (lo, hi) (opt-in) adds aug.scale, one scale per patch of this -- the global -- batch, from draw_scales' own generator
    keyed by jitter_key = (run seed, step): the draws above, and the global streams after them, are what they are without it."""
    B = len(instances)
    aug = Augmentation(B)
    if noise == "host":
        aug.noise = np.zeros((B, S, S, C), dtype=np.float64)
    for b in range(B):
        if np.random.randint(0, 2) == 1:
            aug.rot_on[b] = 1
            aug.rot[b] = rotation_params(instances[b][3], S)
        if np.random.randint(0, 2) == 1:
            aug.noise_on[b] = 1
            if noise == "host":
                aug.noise[b] = np.random.normal(0, 0.01, (S, S, C))
        aug.flip[b] = np.random.randint(0, 3)
    if noise != "host":
        aug.seed = int(np.random.randint(0, 2 ** 31 - 1))
    if scale_jitter is not None:
        aug.scale = draw_scales(B, scale_jitter, jitter_key)
    return aug


# ---------------------------------------------------------------------------------------- device tile pool
class TilePool(object):
    """All tiles (HWC) and label maps (HW) of a split, resident in HBM for the whole run.
    dtype float64 keeps the reference's `img_as_float` precision (bit-exact normalisation); float32
    halves the gather traffic."""

    def __init__(self, tiles, labels, device, dtype=np.float64):
        self.dev = torch.device(device)
        self.C = int(tiles[0].shape[2])
        self.n = len(tiles)
        self.f64 = np.dtype(dtype) == np.float64
        self.h = [int(t.shape[0]) for t in tiles]
        self.w = [int(t.shape[1]) for t in tiles]
        toff = np.cumsum([0] + [t.size for t in tiles])[:-1].astype(np.int64)
        loff = np.cumsum([0] + [t.shape[0] * t.shape[1] for t in tiles])[:-1].astype(np.int64)
        flat = np.concatenate([np.ascontiguousarray(t, dtype=dtype).reshape(-1) for t in tiles])
        if labels is None:
            labels = [np.zeros(t.shape[:2], dtype=np.uint8) for t in tiles]
        lflat = np.concatenate([np.ascontiguousarray(l).astype(np.uint8).reshape(-1) for l in labels])
        self.tiles = torch.from_numpy(flat).to(self.dev)
        self.labels = torch.from_numpy(lflat).to(self.dev)
        self.tile_off = torch.from_numpy(toff).to(self.dev)
        self.lab_off = torch.from_numpy(loff).to(self.dev)
        self.tile_h = torch.tensor(self.h, dtype=torch.int32, device=self.dev)
        self.tile_w = torch.tensor(self.w, dtype=torch.int32, device=self.dev)

    def label_counts(self, K, void_label=None):
        """Per-class pixel counts n_k, k < K, over every label map of the pool (int64 [K]), counted on the device where the maps are
        resident (drs_label_histogram: integer atomics, exact); pixels equal to void_label (None / negative: none) or >= K are left
        out.  Synchronises."""
        K = int(K)
        if not 1 <= K <= MAX_CLASSES:
            raise ValueError("label counts: %d classes, the kernel carries 1..%d" % (K, MAX_CLASSES))
        void = -1 if void_label is None or int(void_label) < 0 else int(void_label)
        counts = torch.zeros(K, dtype=torch.int64, device=self.dev)
        _lib.call("drs_label_histogram", self.labels.data_ptr(), int(self.labels.numel()), K, void, counts.data_ptr(),
                  torch.cuda.current_stream(self.dev).cuda_stream)
        return counts.cpu().numpy()


def _shift_inside(inst_xy, pool, S):
    """isprs:260-269: a window clipped by the bottom/right border is moved back to end at the border."""
    inst = np.asarray(inst_xy, dtype=np.int64)[:, :3].copy()
    hh = np.asarray(pool.h)[inst[:, 0]]
    ww = np.asarray(pool.w)[inst[:, 0]]
    if np.any(hh < S) or np.any(ww < S):
        raise ValueError("Error: Current PATCH size exceeds the tile")       # reference prints and returns None
    inst[:, 1] = np.minimum(inst[:, 1], hh - S)
    inst[:, 2] = np.minimum(inst[:, 2], ww - S)
    return inst


def jitter_centre(r, S, s, n):
    """One axis of the centre rule of the scale-jitter crop (include/drs.h): the patch starts at pixel r (after the shift-back) on a map
    axis of n pixels; c = r + S / 2, clamped to [a, n - a] with a = S / (2 s) when the footprint fits (2 a <= n), else n / 2."""
    c = float(r) + float(S) / 2.0
    a = float(S) / (2.0 * float(s))
    if 2.0 * a <= float(n):
        return min(max(c, a), float(n) - a)
    return float(n) / 2.0


def scale_geometry(inst_xy, pool, S, scale):
    """The footprints geo [B][3] = (step, cy, cx) (float64) of the patches `inst_xy` rows (map, x, y[, ...]) of side S at the scales
    `scale` [B]: step = 1 / s in fp64, the centre from today's shift-back (_shift_inside) and jitter_centre per axis."""
    inst = _shift_inside(inst_xy, pool, S)
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    if len(scale) != len(inst):
        raise ValueError("scale jitter: %d scales for %d patches" % (len(scale), len(inst)))
    geo = np.zeros((len(inst), 3), dtype=np.float64)
    for b, (m, x, y) in enumerate(inst):
        s = float(scale[b])
        if not (math.isfinite(s) and s > 0.0):
            raise ValueError("scale jitter: scale %r of patch %d" % (s, b))
        geo[b] = (1.0 / s, jitter_centre(x, S, s, pool.h[m]), jitter_centre(y, S, s, pool.w[m]))
    return geo


class _Staging(object):
    """Per-step index / augmentation tables go to the device in ONE asynchronous copy from a pinned ring buffer
    (pageable uploads would block the host every step and keep it from running ahead of the GPU).
    Layout per slot, 8-byte aligned: rot f64 [B][6] | inst i32 [B][4] | rot_on u8 [B] | noise_on u8 [B] | pad to 8 | geo f64 [B][3]
    (geo: the footprints of the scale-jitter crop, 24 bytes per patch, written only when the batch has them)."""
    SLOTS = 4

    def __init__(self, dev, b_max):
        self.b_max = b_max
        self.o_rot, self.o_inst = 0, 48 * b_max
        self.o_ron, self.o_non = 64 * b_max, 65 * b_max
        self.o_geo = (66 * b_max + 7) // 8 * 8
        self.nbytes = self.o_geo + 24 * b_max
        self.host = [torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available()) for _ in range(self.SLOTS)]
        self.dev = [torch.empty(self.nbytes, dtype=torch.uint8, device=dev) for _ in range(self.SLOTS)]
        self.events = [None] * self.SLOTS
        self.i = 0

    def upload(self, inst, aug):
        k = self.i
        self.i = (k + 1) % self.SLOTS
        if self.events[k] is not None:
            self.events[k].synchronize()              # the copy issued SLOTS steps ago has long finished
        B = len(inst)
        h = self.host[k].numpy()
        h[self.o_inst:self.o_inst + 4 * inst.size].view(np.int32)[:] = inst.reshape(-1)      # [B][4], or [B][3] (crop_dihedral_to_net)
        if aug is not None:
            h[self.o_rot:self.o_rot + 48 * B].view(np.float64)[:] = aug.rot.reshape(-1)
            h[self.o_ron:self.o_ron + B] = aug.rot_on
            h[self.o_non:self.o_non + B] = aug.noise_on
            if aug.geo is not None:
                h[self.o_geo:self.o_geo + 24 * B].view(np.float64)[:] = np.asarray(aug.geo, dtype=np.float64).reshape(-1)
        self.dev[k].copy_(self.host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev
        base = self.dev[k].data_ptr()
        return base + self.o_inst, base + self.o_rot, base + self.o_ron, base + self.o_non, base + self.o_geo


def _crop_setup(net, B, S, inst, mean, std, aug=None):
    """What the three crop_*_to_net share: the size check, `inst` (int32 [B][3 or 4]) and the augmentation tables uploaded through the
    net's pinned staging ring (_Staging.upload's five device addresses), and mean / std as three C doubles each (bands past the third are
    not normalised; HOST pointers: copied into the kernel arguments).  Returns (addresses, mean3, std3, keep); keep holds the doubles
    alive over the call."""
    import ctypes as C
    net._check(B, S)
    stg = getattr(net, "_staging", None)
    if stg is None:
        stg = net._staging = _Staging(net.dev, net.b_max)
    ptrs = stg.upload(inst, aug)
    m = list(np.asarray(mean, dtype=np.float64)[:3]) + [0.0] * max(0, 3 - len(mean))
    sd = list(np.asarray(std, dtype=np.float64)[:3]) + [1.0] * max(0, 3 - len(std))
    keep = (C.c_double * 3)(*m), (C.c_double * 3)(*sd)
    return ptrs, C.cast(keep[0], C.c_void_p), C.cast(keep[1], C.c_void_p), keep


def crop_to_net(net, pool, instances, S, mean, std, aug=None, void_label=-1, quantize_f16=False):
    """dynamically_create_patches + normalize_images (isprs:1742-1745 / 1579-1583) fused on the device:
    fills net's conv1 slab, net.labels and net.acc_mask for `instances` rows (map, x, y[, rot]).
    quantize_f16: the coffee script's training patches pass through float16 (coffee:293) and are normalised in place in that
    array (coffee:1290): value, difference and quotient are each rounded to float16; NumPy >= 2 evaluates the difference and the
    quotient in the type of the mean / std scalars when that is wider: float32 for coffee's own statistics (np.mean / np.std of
    float32 patches, coffee:78-79), float64 when `mean` arrives as float64 (drs_crop_normalize modes 1 / 2).
    aug.geo set (scale_geometry of aug.scale; opt-in, training only): every patch is resampled from its footprint
    (drs_crop_normalize_scaled, include/drs.h); not set: the plain crop, as ever."""
    B = len(instances)
    inst = np.zeros((B, 4), dtype=np.int32)
    inst[:, :3] = _shift_inside(instances, pool, S)
    if aug is not None:
        inst[:, 3] = aug.flip
    scaled = aug is not None and aug.geo is not None
    if scaled and np.asarray(aug.geo).shape != (B, 3):
        raise ValueError("scale jitter: geo %r for %d patches" % (np.asarray(aug.geo).shape, B))
    (p_inst, p_rot, p_ron, p_non, p_geo), m3, s3, keep = _crop_setup(net, B, S, inst, mean, std, aug)
    noise = None
    if aug is not None and aug.noise is not None:
        noise = torch.from_numpy(aug.noise).to(net.dev)          # reference-exact host noise (tests / parity runs)
    slab, P, ld = net.input_slab()
    head = (pool.tiles.data_ptr(), 1 if pool.f64 else 0, pool.labels.data_ptr(),
            pool.tile_off.data_ptr(), pool.lab_off.data_ptr(), pool.tile_h.data_ptr(), pool.tile_w.data_ptr())
    tail = (p_rot if aug is not None else None, p_ron if aug is not None else None,
            None if noise is None else noise.data_ptr(), p_non if aug is not None else None,
            aug.seed if aug is not None else 0, aug.index0 if aug is not None else 0, m3, s3, B, S, P, ld,
            slab.data_ptr(), net.labels.data_ptr(), net.acc_mask.data_ptr(), int(void_label),
            (2 if getattr(mean, "dtype", None) == np.float64 else 1) if quantize_f16 else 0, net._stream())
    if scaled:                                                   # training with scale jitter: the resampling sibling of the crop
        _lib.call("drs_crop_normalize_scaled", *head, len(pool.h), pool.C, p_inst, p_geo, *tail)
    else:
        _lib.call("drs_crop_normalize", *head, pool.C, p_inst, *tail)
    net._keep = noise                                            # alive until the stream has consumed it
    return inst[:, 1:3]


def _crop_tiles_to_net(net, pool, instances, T, mean, std, g, grid=None):
    """crop_dihedral_to_net (grid None: drs_crop_dihedral) and crop_resampled_to_net (grid = (hs, ws): drs_crop_resampled), which differ
    in that one call: the tiles' (map, row, col) rows as int32 through the staging ring, no shift-back, labels, mask or augmentation"""
    B = len(instances)
    inst = np.ascontiguousarray(np.asarray(instances, dtype=np.int64)[:, :3].astype(np.int32))
    ptrs, m3, s3, keep = _crop_setup(net, B, T, inst, mean, std)
    slab, P, ld = net.input_slab()
    head = (pool.tiles.data_ptr(), 1 if pool.f64 else 0, pool.tile_off.data_ptr(), pool.tile_h.data_ptr(), pool.tile_w.data_ptr(),
            len(pool.h), pool.C, ptrs[0])
    tail = (int(g), m3, s3, B, T, P, ld, slab.data_ptr(), net._stream())
    if grid is None:
        _lib.call("drs_crop_dihedral", *head, *tail)
    else:
        _lib.call("drs_crop_resampled", *head, int(grid[0]), int(grid[1]), *tail)


def crop_dihedral_to_net(net, pool, instances, T, mean, std, g):
    """The test-time-augmentation crop beside crop_to_net (loops.predict_tile_dense with tta): fills net's conv1 slab with the T x T
    tiles at `instances` rows (map, row, col), each transformed by the dihedral code g (dihedral_apply) and normalised as crop_to_net
    normalises (drs_crop_dihedral; no augmentation, labels or mask).  No shift-back: a tile that does not lie inside its map is caught
    on the device and leaves a zero slab."""
    _crop_tiles_to_net(net, pool, instances, T, mean, std, g)


def crop_resampled_to_net(net, pool, instances, T, hs, ws, mean, std, g):
    """The multi-scale crop beside crop_dihedral_to_net (loops.predict_tile_dense with scales): fills net's conv1 slab with the T x T
    tiles at `instances` rows (map, row, col) of the map bilinearly resampled to hs x ws (row / col on that grid), each transformed by
    the dihedral code g and normalised as crop_to_net normalises (drs_crop_resampled; no resized image is made).  A tile that does not
    lie inside the hs x ws grid is caught on the device and leaves a zero slab."""
    _crop_tiles_to_net(net, pool, instances, T, mean, std, g, grid=(hs, ws))


def pack_feed(net, batch_x, batch_y, crop_size, mask=None, acc_mask=None):
    """The reference's feed_dict form (isprs:1746-1752): x float32 [B, s*s*C], y [B, s*s] -> device slab.
    Implemented with the same gather kernel, each patch being its own float32 'tile'."""
    x = np.ascontiguousarray(np.asarray(batch_x, dtype=np.float32))
    B = x.shape[0]
    C_ = net.plan.channels
    S = int(crop_size) if crop_size is not None else int(round(math.sqrt(x.shape[1] // C_)))
    tiles = [x[b].reshape(S, S, C_) for b in range(B)]
    labs = None
    if batch_y is not None:
        labs = [np.asarray(batch_y[b]).reshape(S, S).astype(np.uint8) for b in range(B)]
    pool = TilePool(tiles, labs, net.dev, dtype=np.float32)
    inst = np.stack([np.arange(B), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)], axis=1)
    crop_to_net(net, pool, inst, S, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    M = B * S * S
    if mask is not None:
        net.loss_mask[:M].copy_(torch.from_numpy(np.asarray(mask).reshape(-1).astype(np.uint8)))
    if acc_mask is not None:
        net.acc_mask[:M].copy_(torch.from_numpy(np.asarray(acc_mask).reshape(-1).astype(np.uint8)))
    torch.cuda.current_stream(net.dev).synchronize()      # the temporary pool dies with this frame
    return B, S
