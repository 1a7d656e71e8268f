"""The fp64 statement of the focal training loss (include/drs.h) that the focal-loss tests hold the kernels to; numpy only.
tests/test_focal_loss_plan.py verifies it against torch fp64 autograd on the CPU; tests/test_gpu_focal_loss.py uses it on the device."""
import numpy as np


def focal_closed_form(logits, y, wc, gamma):
    """logits [M][K] (float64), y [M] in [0, K), wc [K], gamma >= 0.  Per pixel, with P = softmax in the max-subtracted form:
        q = 1 - p_t = (sum over k != y, ascending, of ex_k) / se      (never 1 - p_t: no cancellation)
        CE = -log p_t  (as -log1p(-q) below q = 1/8, where log se + max - logit_y has lost its digits)
        m = q^gamma, 0 at q = 0 (gamma > 0)           f = m (1 + gamma p_t r),  r = CE / q -> 1 as q -> 0
    Returns dict(q, pt, ce, m, f, term = wc[y] m CE [M], grad = wc[y] f (P_k - [k == y]) [M][K]); no normaliser applied."""
    lg = np.asarray(logits, dtype=np.float64)
    M, K = lg.shape
    y = np.asarray(y, dtype=np.int64)
    rows = np.arange(M)
    mx = lg.max(axis=1)
    ex = np.exp(lg - mx[:, None])
    se = np.zeros(M)
    so = np.zeros(M)
    for k in range(K):                      # ascending class order
        se = se + ex[:, k]
        so = so + np.where(y == k, 0.0, ex[:, k])
    q = np.minimum(so / se, 1.0)
    pt = ex[rows, y] / se
    ce_log = np.log(se) + mx - lg[rows, y]
    small = q < 0.125
    ce = np.where(small, -np.log1p(-np.where(small, q, 0.0)), ce_log)
    r = np.where(q > 0, ce / np.where(q > 0, q, 1.0), 1.0)
    gamma = float(gamma)
    m = np.ones(M) if gamma == 0.0 else np.where(q > 0, np.power(np.where(q > 0, q, 1.0), gamma), 0.0)
    f = m * (1.0 + gamma * pt * r)
    wy = np.asarray(wc, dtype=np.float64)[y]
    d = ex / se[:, None]
    d[rows, y] = -q                           # P_y - 1 = -q, uncancelled
    return dict(q=q, pt=pt, ce=ce, m=m, f=f, term=wy * m * ce, grad=(wy * f)[:, None] * d)
