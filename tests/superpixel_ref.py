"""The numpy statement of the superpixel vote (include/drs.h drs_superpixel_features / drs_superpixels / drs_region_vote; DESIGN.md
8a.11): byte features in np.float32 steps, SLIC in int64, regions by a plain flood fill, the vote.  NORMATIVE together with the header
text; the device code is held to it bit for bit."""
import numpy as np


# ------------------------------------------------------------------------------------------------------------------ features
def scale_of(tile):
    """the host's choice of (lo, inv) per channel from the map's own minimum and maximum: lo = min, inv = 255 / (max - min) in fp32,
    0 where max == min (the minimum and maximum rounded to fp32 first: rounding is monotonic, so they are those of the fp32 values)"""
    C = tile.shape[-1]
    flat = tile.reshape(-1, C)
    lo, hi = flat.min(axis=0).astype(np.float32), flat.max(axis=0).astype(np.float32)
    with np.errstate(all="ignore"):
        inv = np.where(hi == lo, np.float32(0), np.float32(255) / (hi - lo)).astype(np.float32)
    return lo, inv


def features(tile, lo, inv):
    """uint8 [h][w][C]: t = (v - lo) * inv in two rounded fp32 steps; 0 if !(t > 0), 255 if t >= 255, else rint(t)"""
    with np.errstate(all="ignore"):
        v = tile.astype(np.float32)
        d = (v - np.asarray(lo, dtype=np.float32)).astype(np.float32)
        t = (d * np.asarray(inv, dtype=np.float32)).astype(np.float32)
        out = np.zeros(t.shape, dtype=np.uint8)
        pos = t > 0                                           # False for NaN
        top = pos & (t >= 255)
        mid = pos & ~top
        out[top] = 255
        out[mid] = np.rint(t[mid]).astype(np.uint8)           # half to even, as rintf
    return out


# ------------------------------------------------------------------------------------------------------------------ SLIC
def grid(h, w, S):
    return max(1, h // S), max(1, w // S)


def cells(n, g):
    """the cell of every coordinate 0..n-1 on an axis of g cells"""
    return np.minimum(g - 1, np.arange(n, dtype=np.int64) * g // n)


def slic(feat, S, m, iters):
    """(assign int32 [h][w], colour uint8 [h][w], centres int32 [gh gw][C + 3]) of drs_superpixels"""
    h, w, C = feat.shape
    gh, gw = grid(h, w, S)
    n = gh * gw
    f = feat.astype(np.int64)
    ci, cj = cells(w, gw), cells(h, gh)
    gi, gj = np.arange(gw, dtype=np.int64), np.arange(gh, dtype=np.int64)
    cx = np.tile((2 * gi + 1) * w // (2 * gw), gh)
    cy = np.repeat((2 * gj + 1) * h // (2 * gh), gw)
    F = f[cy, cx]                                             # [n][C]
    count = np.zeros(n, dtype=np.int64)
    ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    for _ in range(iters):
        best = np.full((h, w), np.iinfo(np.int64).max, dtype=np.int64)
        assign = np.full((h, w), -1, dtype=np.int64)
        for dj in (-1, 0, 1):                                 # ascending id: a strict < keeps the lower id on ties
            for di in (-1, 0, 1):
                jj, ii = cj[:, None] + dj, ci[None, :] + di
                ok = (jj >= 0) & (jj < gh) & (ii >= 0) & (ii < gw)
                cid = np.clip(jj, 0, gh - 1) * gw + np.clip(ii, 0, gw - 1)
                key = S * S * ((f - F[cid]) ** 2).sum(axis=2) + m * m * ((xs - cx[cid]) ** 2 + (ys - cy[cid]) ** 2)
                assert key.max() < 1 << 32
                take = ok & (key < best)
                best[take] = key[take]
                assign[take] = cid[take]
        flat = assign.reshape(-1)
        count = np.bincount(flat, minlength=n).astype(np.int64)
        sx, sy = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        sf = np.zeros((n, C), dtype=np.int64)
        np.add.at(sx, flat, np.broadcast_to(xs, (h, w)).reshape(-1))
        np.add.at(sy, flat, np.broadcast_to(ys, (h, w)).reshape(-1))
        np.add.at(sf, flat, f.reshape(-1, C))
        assert max(sx.max(), sy.max(), sf.max()) < 1 << 32
        live = count > 0
        d = 2 * count[live]
        cx, cy, F = cx.copy(), cy.copy(), F.copy()
        cx[live] = (2 * sx[live] + count[live]) // d
        cy[live] = (2 * sy[live] + count[live]) // d
        F[live] = (2 * sf[live] + count[live][:, None]) // d[:, None]
    colour = ((assign // gw) % 4 * 4 + (assign % gw) % 4).astype(np.uint8)
    centres = np.concatenate([cx[:, None], cy[:, None], F, count[:, None]], axis=1).astype(np.int32)
    return assign.astype(np.int32), colour, centres


# ------------------------------------------------------------------------------------------------------------------ regions
def regions(ids):
    """(label int32, size int32) [h][w] of the 4-connected pieces of equal values of ids, by a plain flood fill: label = the smallest
    linear index of the piece -- what drs_components(.., 4) writes for a map whose 4-adjacent bytes differ exactly where ids differ"""
    h, w = ids.shape
    label = np.full((h, w), -1, dtype=np.int32)
    size = np.zeros((h, w), dtype=np.int32)
    for y0 in range(h):
        for x0 in range(w):
            if label[y0, x0] >= 0:
                continue
            root, v = y0 * w + x0, ids[y0, x0]                # row-major scan: the first pixel met is the smallest index
            label[y0, x0] = root
            stack, members = [(y0, x0)], [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < h and 0 <= xx < w and label[yy, xx] < 0 and ids[yy, xx] == v:
                        label[yy, xx] = root
                        stack.append((yy, xx))
                        members.append((yy, xx))
            for y, x in members:
                size[y, x] = len(members)
    return label, size


# ------------------------------------------------------------------------------------------------------------------ the vote
def vote(m, label, K, weight=None):
    """(the voted map uint8 [h][w], [regions, changed pixels]) of drs_region_vote"""
    out = m.copy()
    flat, lab = m.reshape(-1), label.reshape(-1)
    wt = np.ones(flat.shape, dtype=np.int64) if weight is None else weight.reshape(-1).astype(np.int64)
    order = np.argsort(lab, kind="stable")
    roots, starts = np.unique(lab[order], return_index=True)
    ends = list(starts[1:]) + [len(order)]
    o = out.reshape(-1)
    for s, e in zip(starts, ends):
        px = order[s:e]
        votes = flat[px] < K
        V = np.zeros(K, dtype=np.int64)
        np.add.at(V, flat[px][votes], wt[px][votes])
        if V.max() > 0:
            o[px[votes]] = int(np.argmax(V))                  # the first maximum: ties to the lower class
    return out, [int(len(roots)), int((out != m).sum())]


# ------------------------------------------------------------------------------------------------------------------ test images
def image(h, w, C, seed, kind="blobs"):
    """float32 [h][w][C] test images: smooth blobs plus noise; a constant; a period-3 two-valued checker; white noise, uniform
    and two-valued"""
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full((h, w, C), 0.25, dtype=np.float32)
    if kind == "checker3":
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((y // 3 + x // 3) % 2).astype(np.float32))[:, :, None], C, axis=2).copy()
    if kind == "noise":
        return rng.random((h, w, C), dtype=np.float32)
    if kind == "noise2":
        return rng.integers(0, 2, size=(h, w, C)).astype(np.float32)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    out = np.zeros((h, w, C), dtype=np.float32)
    for c in range(C):
        a, b, p = rng.uniform(0.05, 0.3, size=3)
        out[:, :, c] = np.sign(np.sin(a * x + p) * np.cos(b * y + c)) * 0.5 + 0.1 * rng.standard_normal((h, w))
    return out.astype(np.float32)


def label_map(h, w, K, seed, beyond=False):
    """a random uint8 map of K classes in small blocks with speckle; beyond: some bytes >= K"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, K, size=((h + 4) // 5, (w + 6) // 7), dtype=np.uint8)
    m = np.kron(coarse, np.ones((5, 7), dtype=np.uint8))[:h, :w].copy()
    speck = rng.random((h, w)) < 0.2
    m[speck] = rng.integers(0, K, size=int(speck.sum()), dtype=np.uint8)
    if beyond:
        far = rng.random((h, w)) < 0.1
        m[far] = rng.integers(K, 256, size=int(far.sum()), dtype=np.uint8)
    return m
