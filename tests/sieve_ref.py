"""The connected components, the sieve round, the sieve and the object census of DESIGN.md 8a.8 / include/drs.h (drs_components,
drs_sieve_round, drs_component_census; loops.sieve_labels) stated in numpy.  Integer arithmetic throughout; numpy only.

  component    a maximal c-connected (c = 4 or 8) set of pixels with the same byte; the edge of the map connects nothing
  label[p]     the smallest linear index y w + x of p's component (int32);   size[p] its pixel count (uint32), at every pixel
  small        byte b < K and size < min_size[b]
  one round    every small component S looks at the pairs (p in S, q a FOUR-neighbour of p inside the map) with m[q] != m[p],
               m[q] < K and q's component not small; S takes the byte of the largest key (size[q], 255 - m[q]); all at once
  the sieve    components, then a round; again until a round merges nothing or SIEVE_MAX_ROUNDS rounds have run
  census       table[byte][floor(log2(size))] += 1 per component of a byte < K"""
import numpy as np

import boundary_ref

SIEVE_MAX_ROUNDS = 64


def _pairs(h, w, connectivity):
    """(p, q) linear indices of every neighbouring pair inside the map, each pair once (q after p in row-major order)"""
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    out = [(idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])]
    if connectivity == 8:
        out += [(idx[:-1, :-1], idx[1:, 1:]), (idx[:-1, 1:], idx[1:, :-1])]
    return np.concatenate([a.reshape(-1) for a, _ in out]), np.concatenate([b.reshape(-1) for _, b in out])


def components(m, connectivity):
    """(label int32 [h][w], size uint32 [h][w]).  Every pixel starts as its own label; every pair of neighbours with the same byte
    pulls the labels their two labels point to down to the smaller of the two, and every label then follows its label, until nothing
    moves.  A label never exceeds its pixel's index and never leaves the component, so at the fixed point -- equal across every pair,
    each label its own label -- it is the component's smallest index."""
    assert connectivity in (4, 8)
    m = np.asarray(m)
    h, w = m.shape
    p, q = _pairs(h, w, connectivity)
    same = m.reshape(-1)[p] == m.reshape(-1)[q]
    p, q = p[same], q[same]
    lab = np.arange(h * w, dtype=np.int64)
    while True:
        before = lab.copy()
        low = np.minimum(lab[p], lab[q])
        np.minimum.at(lab, lab[p], low)
        np.minimum.at(lab, lab[q], low)
        np.minimum.at(lab, p, low)
        np.minimum.at(lab, q, low)
        while True:
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt
        if (lab == before).all():
            break
    size = np.bincount(lab, minlength=h * w)[lab]
    return lab.astype(np.int32).reshape(h, w), size.astype(np.uint32).reshape(h, w)


def _thresholds(K, min_size):
    ms = np.full(K, int(min_size), dtype=np.int64) if np.isscalar(min_size) else np.asarray(min_size, dtype=np.int64)
    assert ms.shape == (K,) and (ms >= 0).all()
    return ms


def small_mask(m, size, K, min_size):
    ms = _thresholds(K, min_size)
    ok = m < K
    out = np.zeros(m.shape, dtype=bool)
    out[ok] = size[ok].astype(np.int64) < ms[m[ok].astype(np.int64)]
    return out


def sieve_round(m, K, min_size, connectivity):
    """one round: (the new map, [small components at the start, those of them that merged])"""
    m = np.asarray(m)
    h, w = m.shape
    label, size = components(m, connectivity)
    small = small_mask(m, size, K, min_size)
    mf, lf, sf, smf = m.reshape(-1).astype(np.int64), label.reshape(-1).astype(np.int64), size.reshape(-1).astype(np.int64), small.reshape(-1)
    a, b = _pairs(h, w, 4)                                                 # the four edge neighbours, whatever the connectivity
    p, q = np.concatenate([a, b]), np.concatenate([b, a])                  # both directions
    offers = smf[p] & (mf[q] != mf[p]) & (mf[q] < K) & ~smf[q]
    p, q = p[offers], q[offers]
    best = np.zeros(h * w, dtype=np.int64)                                 # at the component's label; 0 = no offer (a key is >= 256)
    np.maximum.at(best, lf[p], sf[q] * 256 + (255 - mf[q]))
    key = best[lf]
    take = smf & (key > 0)
    out = mf.copy()
    out[take] = 255 - (key[take] & 255)
    roots = lf == np.arange(h * w)
    return out.astype(np.uint8).reshape(h, w), [int((roots & smf).sum()), int((roots & take).sum())]


def census(m, label, size, K):
    """table [K][32] int64"""
    m, label, size = np.asarray(m).reshape(-1), np.asarray(label).reshape(-1), np.asarray(size).reshape(-1)
    roots = (label == np.arange(m.size)) & (m < K)
    table = np.zeros((K, 32), dtype=np.int64)
    bins = np.array([int(s).bit_length() - 1 for s in size[roots]], dtype=np.int64)
    np.add.at(table, (m[roots].astype(np.int64), bins), 1)
    return table


def sieve(m, K, min_size, connectivity, max_rounds=SIEVE_MAX_ROUNDS):
    """(the sieved map, info) -- info as loops.sieve_labels returns it.  rounds counts every round that ran, the last one, which
    merged nothing, included; capped: the loop ended because max_rounds had run, not because a round merged nothing."""
    m = np.asarray(m)
    cur = m.copy()
    before = census(cur, *components(cur, connectivity), K).sum(axis=1)
    rounds = merged = 0
    capped = False
    while True:
        nxt, (n_small, n_merged) = sieve_round(cur, K, min_size, connectivity)
        rounds += 1
        merged += n_merged
        cur = nxt
        if n_merged == 0:
            break
        if rounds == max_rounds:
            capped = True
            break
    label, size = components(cur, connectivity)
    left = int(((label.reshape(-1) == np.arange(m.size)) & small_mask(cur, size, K, min_size).reshape(-1)).sum())
    after = census(cur, label, size, K).sum(axis=1)
    info = {"rounds": rounds, "merged": merged, "left_small": left, "changed_pixels": int((cur != m).sum()),
            "objects_before": [int(v) for v in before], "objects_after": [int(v) for v in after], "capped": capped}
    return cur, info


# ---------------------------------------------------------------------------------------------------------------- inputs
def speckled(h, w, K, seed=0, frac=0.15):
    """a realistic speckled map: boundary_ref.synthetic_case's blob map with `frac` of the pixels re-drawn uniformly from 0..K-1"""
    truth, _ = boundary_ref.synthetic_case(h, w, K, seed)
    rng = np.random.default_rng(seed + 1000)
    hit = rng.random((h, w)) < frac
    out = truth.copy()
    out[hit] = rng.integers(0, K, size=int(hit.sum())).astype(np.uint8)
    return out


def uniform(h, w, byte=2):
    return np.full((h, w), byte, dtype=np.uint8)


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) & 1).astype(np.uint8)


def serpentine(h, w):
    """one corridor of byte 1, one pixel wide, through a map of byte 0 walls: every even row is corridor, joined to the next even row
    at alternating ends -- a single 4-connected component whose pixels in row-major order are far from their order along the path"""
    m = np.zeros((h, w), dtype=np.uint8)
    m[0::2] = 1
    for i, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            m[y, w - 1 if i % 2 == 0 else 0] = 1
    return m


def rings(n=5):
    """a single pixel and n one-pixel rings around it (Chebyshev distance 1..n), bytes alternating 1, 2, in a field of byte 0 that is
    the only non-small region at min_size 200: a round peels one ring, from the outside in"""
    side = 2 * n + 11
    c = side // 2
    yy, xx = np.mgrid[0:side, 0:side]
    d = np.maximum(abs(yy - c), abs(xx - c))
    return np.where(d > n, 0, 1 + (d & 1)).astype(np.uint8)


def noise(h=64, w=64, K=4, seed=7):
    return np.random.default_rng(seed).integers(0, K, size=(h, w)).astype(np.uint8)
