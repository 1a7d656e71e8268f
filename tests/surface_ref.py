"""The exact distance transform and the surface-distance table of DESIGN.md 8a.10 / include/drs.h (drs_distance_transform,
drs_surface_histogram) stated in numpy, brute force, straight from the definitions: the minimum over the list of sites, for every pixel.
Integer arithmetic throughout (int64 / Python ints; math.isqrt for the two roots of the table).

  b[p]    = veil_label where veil[p] == veil_label, else map[p]
  sites   = CLASS: b == cls;  NOT_CLASS: b != cls;  CONTOUR: b == cls and some 4-neighbour INSIDE the map carries another byte
  d2[p]   = min over the sites q of |p - q|^2, INF without a site
  table[dir][c][...]: direction 0 walks the CONTOUR set of c in truth with D to that of c in pred' (pred veiled by truth at ignore),
      direction 1 the reverse; counterpart empty: [BINS + 1] += 1; else [min(b, BINS - 1)] += 1 and [BINS] += f with
      b = the smallest integer with 16 D <= b^2, f = isqrt(D 2^20)

The edge of the map is not a boundary; a byte is just a byte."""
import math

import numpy as np

from boundary_ref import _voronoi

CLASS, NOT_CLASS, CONTOUR = 0, 1, 2
INF = 0x7FFFFFFF
BINS = 4096


def veiled(m, veil=None, veil_label=None):
    m = np.asarray(m)
    if veil is None:
        return m
    out = m.copy()
    out[np.asarray(veil) == veil_label] = veil_label
    return out


def sites(m, mode, cls, veil=None, veil_label=None):
    """bool [h][w]: the sites of the transform"""
    b = veiled(m, veil, veil_label)
    if mode == CLASS:
        return b == cls
    if mode == NOT_CLASS:
        return b != cls
    other = np.zeros(b.shape, dtype=bool)                                 # some neighbour inside the map is not cls
    other[1:] |= b[:-1] != cls
    other[:-1] |= b[1:] != cls
    other[:, 1:] |= b[:, :-1] != cls
    other[:, :-1] |= b[:, 1:] != cls
    return (b == cls) & other


def distance2_to(mask, chunk=512):
    """int64 [h][w]: the squared distance of every pixel to the nearest True of mask, INF without one; the site list in chunks"""
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    qy, qx = [v.astype(np.int64) for v in np.nonzero(mask)]
    best = np.full((h, w), INF, dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    for s in range(0, len(qy), chunk):
        d = (yy[..., None] - qy[s:s + chunk]) ** 2 + (xx[..., None] - qx[s:s + chunk]) ** 2
        best = np.minimum(best, d.min(axis=-1))
    return best


def distance2(m, mode, cls, veil=None, veil_label=None):
    return distance2_to(sites(m, mode, cls, veil, veil_label))


def bin_of(D):
    """the smallest integer b with 16 D <= b^2"""
    r = math.isqrt(16 * D)
    return r if r * r == 16 * D else r + 1


def contour_sets(truth, pred, c, ignore):
    """(S_t(c), S_p(c)) as bool maps"""
    truth, pred = np.asarray(truth), np.asarray(pred)
    if ignore is None or ignore < 0:
        return sites(truth, CONTOUR, c), sites(pred, CONTOUR, c)
    return sites(truth, CONTOUR, c), sites(pred, CONTOUR, c, truth, ignore)


def table(truth, pred, K, ignore):
    """the table [2][K][BINS + 2], int64"""
    ignore = -1 if ignore is None else ignore
    out = np.zeros((2, K, BINS + 2), dtype=np.int64)
    for c in range(K):
        if c == ignore:
            continue
        st, sp = contour_sets(truth, pred, c, ignore)
        for direction, (walk, other) in enumerate(((st, sp), (sp, st))):
            if not walk.any():
                continue
            if not other.any():
                out[direction, c, BINS + 1] += int(walk.sum())
                continue
            for D in distance2_to(other)[walk].tolist():
                out[direction, c, min(bin_of(D), BINS - 1)] += 1
                out[direction, c, BINS] += math.isqrt(D << 20)
    return out


def synthetic_case(h, w, K, seed, ignore=-1, shift=3):
    """(truth, pred): two correlated blob maps, uint8 [h][w], in the manner of boundary_ref.synthetic_case: a Voronoi map of a few
    seeds plus two small objects the prediction misses; with 0 <= ignore the pixels of the truth that touch another class carry
    `ignore`; the prediction is the same Voronoi map with every seed displaced by up to `shift` pixels plus a few speckles."""
    rng = np.random.default_rng(seed)
    ns = max(2, min(12, h * w // 1000 + 2))
    pts = np.stack([rng.integers(0, h, ns), rng.integers(0, w, ns)], axis=1)
    labels = (rng.permutation(ns) % K).astype(np.uint8)
    labels[:2] = (0, 1)
    truth = _voronoi(h, w, pts, labels)
    for _ in range(2):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        truth[y:y + 3, x:x + 3] = (truth[y, x] + 1) % K
    if ignore >= 0:
        edge = np.zeros((h, w), dtype=bool)
        edge[1:] |= truth[1:] != truth[:-1]
        edge[:-1] |= truth[:-1] != truth[1:]
        edge[:, 1:] |= truth[:, 1:] != truth[:, :-1]
        edge[:, :-1] |= truth[:, :-1] != truth[:, 1:]
        truth[edge] = ignore
    pred = _voronoi(h, w, pts + rng.integers(-shift, shift + 1, size=pts.shape), labels)
    for _ in range(max(1, h * w // 2500)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pred[y, x] = (pred[y, x] + 1 + int(rng.integers(0, K - 1))) % K
    return truth, pred
