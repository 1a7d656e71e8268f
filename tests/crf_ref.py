"""The local dense-CRF refinement (include/drs.h: drs_crf_unary, drs_crf_step) restated in fp64 numpy: the
reference of tests/test_gpu_crf.py and the subject of the property tests in tests/test_crf_plan.py.  One module-level statement per
line of the rule; no device, no torch."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
DEFAULTS = dict(iters=5, radius=5, step=2, w_app=4.0, theta_xy=8.0, theta_rgb=0.08, w_smooth=2.0, theta_s=2.0)


def unary(sums, occur, sums_are_prob, beta=1.0):
    """sums [h, w, K] (float32 values), occur [h, w] -> (logp [h, w, K] fp64, Q0 [h, w, K] fp64, live [h, w] bool).  The score vector u
    is the fp32 quotient sums / occur (occur 0 counts as 1), for probabilities the log of that quotient clamped at FLT_MIN."""
    s = np.asarray(sums, dtype=np.float32)
    oc = np.asarray(occur).astype(np.int64)
    live = oc > 0
    q = (s / np.where(live, oc, 1).astype(np.float32)[..., None]).astype(np.float32)
    u = np.log(np.maximum(q.astype(np.float64), FLT_MIN)) if sums_are_prob else q.astype(np.float64)
    t = float(beta) * u
    t = t - t.max(axis=-1, keepdims=True)
    logp = t - np.log(np.exp(t).sum(axis=-1, keepdims=True))
    return logp, np.exp(logp), live


def _shift(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the map, 0 elsewhere"""
    h, w = a.shape[:2]
    b = np.zeros_like(a)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        b[yd, xd] = a[ys, xs]
    return b


def mean_field_step(q, logp, live, tile, radius, step, w_app, theta_xy, theta_rgb, w_smooth, theta_s):
    """One iteration: q [h, w, K] -> the next Q (fp64).  tile [h, w, C]: its values as stored, read as fp32."""
    q = np.asarray(q, dtype=np.float64)
    f = np.asarray(tile).astype(np.float32).astype(np.float64)
    live = np.asarray(live, dtype=bool)
    inside = np.ones(live.shape, dtype=bool)
    m = np.zeros_like(q)
    for i in range(-radius, radius + 1):              # the fixed order of the sum: i ascending, then j ascending
        for j in range(-radius, radius + 1):
            if i == 0 and j == 0:
                continue
            dy, dx = i * step, j * step
            counts = _shift(live & inside, dy, dx)    # the neighbour is inside the map and live
            d2 = float(dy * dy + dx * dx)
            df = f - _shift(f, dy, dx)
            kap = (w_app * np.exp(-d2 / (2.0 * theta_xy ** 2) - (df * df).sum(axis=-1) / (2.0 * theta_rgb ** 2))
                   + w_smooth * np.exp(-d2 / (2.0 * theta_s ** 2)))
            m += np.where(counts, kap, 0.0)[..., None] * _shift(q, dy, dx)
    z = logp + m
    z = z - z.max(axis=-1, keepdims=True)
    e = np.exp(z)
    out = e / e.sum(axis=-1, keepdims=True)
    return np.where(live[..., None], out, q)          # a dead pixel never moves


def refine(sums, occur, sums_are_prob, tile, iters=5, radius=5, step=2, w_app=4.0, theta_xy=8.0, theta_rgb=0.08, w_smooth=2.0,
           theta_s=2.0, beta=1.0):
    """Q after `iters` iterations (fp64 [h, w, K]) and the live map."""
    logp, q, live = unary(sums, occur, sums_are_prob, beta)
    for _ in range(iters):
        q = mean_field_step(q, logp, live, tile, radius, step, w_app, theta_xy, theta_rgb, w_smooth, theta_s)
    return q, live


def labels(q):
    """first maximum over the classes"""
    return np.argmax(q, axis=-1).astype(np.uint8)


def top2_margin(q):
    s = np.sort(q, axis=-1)
    return s[..., -1] - s[..., -2]


def score_bytes(q, live):
    """drs_stitch_finalize_scores on (Q, live, sums_are_prob = 1): confidence, margin, entropy as bytes, in fp64 (a byte may differ by
    one from the device's fp32 at a rounding boundary).  A dead pixel: 0, 0, 255."""
    K = q.shape[-1]
    lab = np.argmax(q, axis=-1)
    top = np.take_along_axis(q, lab[..., None], axis=-1)[..., 0]
    rest = q.copy()
    np.put_along_axis(rest, lab[..., None], -np.inf, axis=-1)
    second = rest.max(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(q > 0, q * np.log(q), 0.0).sum(axis=-1) / np.log(K)

    def byte(s):
        return np.floor(255.0 * np.clip(s, 0.0, 1.0) + 0.5).astype(np.uint8)
    out = {"confidence": byte(top), "margin": byte(top - second), "entropy": byte(ent)}
    dead = {"confidence": 0, "margin": 0, "entropy": 255}
    return {k: np.where(live, v, dead[k]).astype(np.uint8) for k, v in out.items()}


def synthetic_case(h, w, K, C, seed=0, prob=False, dead=3):
    """The inputs of the tests: block-constant truth, one colour per class and band plus sigma = 0.04 noise, logits N(0, 1.5) +
    2 onehot (or, with prob, the sum of two softmax vectors over occur = 2), and a dead (occur = 0, sums = 0) dead x dead corner."""
    rng = np.random.default_rng(seed)
    by, bx = max(2, h // 3), max(2, w // 4)
    truth = rng.integers(0, K, size=(-(-h // by), -(-w // bx)))
    truth = np.repeat(np.repeat(truth, by, axis=0), bx, axis=1)[:h, :w]
    colours = rng.uniform(0.1, 0.9, size=(K, C))
    tile = colours[truth] + rng.normal(0.0, 0.04, size=(h, w, C))
    logits = rng.normal(0.0, 1.5, size=(h, w, K)) + 2.0 * np.eye(K)[truth]
    occur = np.full((h, w), 2 if prob else 1, dtype=np.uint32)
    if prob:
        other = logits + rng.normal(0.0, 0.5, size=logits.shape)
        sums = sum(np.exp(z - z.max(-1, keepdims=True)) / np.exp(z - z.max(-1, keepdims=True)).sum(-1, keepdims=True)
                   for z in (logits, other))
    else:
        sums = logits
    sums = sums.astype(np.float32)
    d = min(dead, h, w)
    occur[h - d:, w - d:] = 0
    sums[h - d:, w - d:] = 0.0
    return truth.astype(np.uint8), tile, sums, occur
