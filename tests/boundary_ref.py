"""The boundary-quality counts of DESIGN.md 8a.7 / include/drs.h (drs_boundary_distance, drs_boundary_histogram) stated in numpy,
brute force, straight from the definitions: every offset of the window is tried for every pixel.  Integer arithmetic throughout.

  D2_m(p) = min { dy^2 + dx^2 : |dy| <= R, |dx| <= R, q = p + (dy, dx) inside the map, m[q] != m[p] },  INF without such a q
  bin_m(p) = the smallest i with D2_m(p) <= d_i^2, or n
  hist[bin_truth(p)][bin_pred(p)][truth[p]][pred[p]] += 1  for every p with truth != ignore, truth < K and pred < K

The edge of the map is not a boundary: a position outside the map is never "different".  A byte is just a byte: the ignore label in
the truth, or a byte >= K in the prediction, differs from the class pixels beside it like any other byte."""
import numpy as np

INF = np.iinfo(np.int64).max


def distance2(m, R):
    """D2 of a byte map [h][w] at reach R: int64 [h][w], INF where the window holds no other byte"""
    m = np.asarray(m)
    h, w = m.shape
    best = np.full((h, w), INF, dtype=np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if abs(dy) >= h or abs(dx) >= w:
                continue                                                  # q is outside the map for every p
            # p ranges over the pixels whose q = p + (dy, dx) is inside the map
            ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
            yq, xq = slice(max(0, dy), h - max(0, -dy)), slice(max(0, dx), w - max(0, -dx))
            differs = m[yq, xq] != m[ys, xs]
            view = best[ys, xs]
            view[differs] = np.minimum(view[differs], dy * dy + dx * dx)
    return best


def distance2_u16(m, R):
    """what drs_boundary_distance writes: min(D2, 65535) as uint16"""
    return np.minimum(distance2(m, R), 65535).astype(np.uint16)


def bins(d2, distances):
    """bin of every pixel: the smallest i with D2 <= d_i^2, or n"""
    n = len(distances)
    b = np.full(d2.shape, n, dtype=np.int64)
    for i in range(n - 1, -1, -1):
        b[d2 <= distances[i] * distances[i]] = i
    return b


def counted(truth, pred, K, ignore):
    """the pixels drs_confusion counts"""
    return (truth != ignore) & (truth < K) & (pred < K)


def histogram(truth, pred, K, ignore, distances):
    """the table [(n+1)][(n+1)][K][K], int64"""
    truth, pred = np.asarray(truth), np.asarray(pred)
    n, R = len(distances), distances[-1]
    bt, bp = bins(distance2(truth, R), distances), bins(distance2(pred, R), distances)
    ok = counted(truth, pred, K, ignore)
    hist = np.zeros((n + 1, n + 1, K, K), dtype=np.int64)
    np.add.at(hist, (bt[ok], bp[ok], truth[ok].astype(np.int64), pred[ok].astype(np.int64)), 1)
    return hist


def confusion(truth, pred, K, ignore):
    ok = counted(truth, pred, K, ignore)
    cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(cm, (truth[ok].astype(np.int64), pred[ok].astype(np.int64)), 1)
    return cm


def _voronoi(h, w, pts, labels):
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy[..., None] - pts[:, 0]) ** 2 + (xx[..., None] - pts[:, 1]) ** 2
    return labels[np.argmin(d, axis=-1)].astype(np.uint8)


def synthetic_case(h, w, K, seed, ignore=-1):
    """(truth, pred): two correlated blob maps, uint8 [h][w].  The truth is a Voronoi map of a few seeds (large cells, so that some
    pixels are far from every contour) plus two small objects the prediction misses; with ignore >= 0 the pixels that touch another
    class (4-neighbours) carry `ignore`: a thin band along the boundaries.  The prediction is the same Voronoi map with every seed
    displaced by up to 3 pixels -- displaced contours -- plus a few single-pixel speckles in classes of their own."""
    rng = np.random.default_rng(seed)
    ns = max(2, min(12, h * w // 1000 + 2))
    pts = np.stack([rng.integers(0, h, ns), rng.integers(0, w, ns)], axis=1)
    labels = (rng.permutation(ns) % K).astype(np.uint8)
    labels[:2] = (0, 1)                                                   # at least two classes, whatever the draw
    base = _voronoi(h, w, pts, labels)
    truth = base.copy()
    for _ in range(2):                                                    # small objects in the truth only
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        truth[y:y + 3, x:x + 3] = (truth[y, x] + 1) % K
    if ignore >= 0:
        edge = np.zeros((h, w), dtype=bool)
        edge[1:] |= truth[1:] != truth[:-1]
        edge[:-1] |= truth[:-1] != truth[1:]
        edge[:, 1:] |= truth[:, 1:] != truth[:, :-1]
        edge[:, :-1] |= truth[:, :-1] != truth[:, 1:]
        truth[edge] = ignore
    moved = pts + rng.integers(-3, 4, size=pts.shape)
    pred = _voronoi(h, w, moved, labels)
    for _ in range(max(1, h * w // 2500)):                                # speckle
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        pred[y, x] = (pred[y, x] + 1 + int(rng.integers(0, K - 1))) % K
    return truth, pred
