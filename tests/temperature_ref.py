"""fp64 numpy restatement of temperature scaling (include/drs.h: drs_temperature_stats, drs_stitch_finalize_scores_t),
shared by tests/test_temperature_plan.py (CPU) and tests/test_gpu_temperature.py.  Nothing here touches the device."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)


def score_vectors(sums, occur, is_prob):
    """u [n][K] in fp64 of sums [n][K] (float32 values) and occur [n]: the quotient in fp64 (logits), or the log of the fp32 quotient
    clamped at FLT_MIN (probabilities); occur 0 counts as 1"""
    sums = np.asarray(sums, dtype=np.float32)
    oc = np.where(np.asarray(occur) == 0, 1, np.asarray(occur)).reshape(-1, 1)
    if is_prob:
        q = (sums / oc.astype(np.float32)).astype(np.float32)            # one correctly rounded fp32 division, as the device's
        return np.log(np.maximum(q, np.float32(FLT_MIN)).astype(np.float64))
    return sums.astype(np.float64) / oc.astype(np.float64)


def counted(occur, truth, K, ignore_label):
    occur, truth = np.asarray(occur).reshape(-1), np.asarray(truth).reshape(-1)
    return (occur > 0) & (truth != ignore_label) & (truth < K)


def stats(u, truth, beta, keep=None):
    """(N, L, G, H, A) of the score vectors u [n][K] and labels truth [n] at inverse temperature beta, over the pixels of `keep`"""
    u = np.asarray(u, dtype=np.float64)
    truth = np.asarray(truth).reshape(-1).astype(np.int64)
    if keep is not None:
        u, truth = u[keep], truth[keep]
    if u.shape[0] == 0:
        return (0.0, 0.0, 0.0, 0.0, 0.0)
    t = float(beta) * u
    m = t.max(axis=1)
    e = np.exp(t - m[:, None])
    se = e.sum(axis=1)
    p = e / se[:, None]
    mu = (p * u).sum(axis=1)
    uy = u[np.arange(u.shape[0]), truth]
    L = np.log(se) + m - float(beta) * uy
    H = (p * (u - mu[:, None]) ** 2).sum(axis=1)
    return (float(u.shape[0]), float(L.sum()), float((mu - uy).sum()), float(H.sum()), float(np.abs(mu - uy).sum()))


def golden_section(u, truth, lo=1.0 / 64.0, hi=64.0, iters=200):
    """the minimiser of L over ln beta in [ln lo, ln hi] by golden-section search: no derivative, so independent of the Newton fit"""
    f = lambda x: stats(u, truth, np.exp(x))[1]      # noqa: E731
    a, b = np.log(lo), np.log(hi)
    g = (np.sqrt(5.0) - 1.0) / 2.0
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(iters):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = f(c)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = f(d)
    return float(np.exp(0.5 * (a + b)))


def scores_t(sums, occur, is_prob, beta):
    """(labels, {kind: q}) of drs_stitch_finalize_scores_t at beta != 1: t = float32(beta) * v formed in fp32 (v the fp32 quotient, or
    its fp32 logarithm clamped at FLT_MIN), everything after it in fp64; q = 255 clamp(score) + 0.5, unrounded"""
    sums = np.asarray(sums, dtype=np.float32)
    n, K = sums.shape
    occur = np.asarray(occur).reshape(n)
    oc = np.where(occur == 0, 1, occur)
    lab = (sums.astype(np.float64) / oc.astype(np.float64)[:, None]).argmax(axis=1)
    v = (sums / oc.astype(np.float32)[:, None]).astype(np.float32)
    if is_prob:
        v = np.log(np.maximum(v, np.float32(FLT_MIN)).astype(np.float64)).astype(np.float32)
    t = (np.float32(beta) * v).astype(np.float32).astype(np.float64)
    t = t - t.max(axis=1, keepdims=True)
    e = np.exp(t)
    se = e.sum(axis=1, keepdims=True)
    p = e / se
    rows = np.arange(n)
    conf = p[rows, lab]
    rest = p.copy()
    rest[rows, lab] = -np.inf
    margin = conf - rest.max(axis=1) if K > 1 else conf
    ent = (np.log(se[:, 0]) - (p * t).sum(axis=1)) / np.log(K) if K > 1 else np.zeros(n)
    unc = occur == 0
    s = {"confidence": np.where(unc, 0.0, conf), "margin": np.where(unc, 0.0, margin), "entropy": np.where(unc, 1.0, ent)}
    return lab.astype(np.uint8), {k: 255.0 * np.clip(x, 0.0, 1.0) + 0.5 for k, x in s.items()}
