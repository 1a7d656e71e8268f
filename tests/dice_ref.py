"""The soft Dice / Tversky term of the training loss (include/drs.h, "Training level: soft Dice / Tversky term") stated
in fp64 numpy: the per-(patch, class) soft counts, the coefficients the fused classifier reads, the loss and the closed-form logit
gradient.  tests/test_dice_loss_plan.py holds the closed form against fp64 autograd and finite differences.

For patch b and class c, every sum over the in-loss pixels of that patch only, p = softmax(logits):
    TP = sum p_c [y = c]     SP = sum p_c     N = sum [y = c]     n_b = sum_c N
    D  = TP + alpha (SP - TP) + beta (N - TP) + eps              T = (TP + eps) / D
    L_dice = inv_n sum_b n_b (lam / K) sum_c (1 - T)
    G_in  = -(lam n_b / K) (D - (TP + eps)(1 - beta)) / D^2      G_out = +(lam n_b / K) alpha (TP + eps) / D^2
    g_c = [y = c] ? G_in : G_out         dL_dice / dlogit_k = inv_n P_k (g_k - sum_c P_c g_c)
"""
import numpy as np


def softmax(lg):
    """row-wise softmax of fp64 logits [M, K], max-subtracted"""
    lg = np.asarray(lg, dtype=np.float64)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def in_loss(y, K, loss_mask=None):
    """what "in the loss" means for the cross-entropy: loss_mask set when given, and label < K.  y, loss_mask: [B, n]"""
    y = np.asarray(y)
    ok = y < K
    return ok if loss_mask is None else ok & (np.asarray(loss_mask) != 0)


def stats(p, y, inl, K):
    """p [B, n, K] probabilities, y [B, n] labels, inl [B, n] bool -> (TP, SP, N), each [B, K] float64"""
    B = p.shape[0]
    tp, sp, cnt = np.zeros((B, K)), np.zeros((B, K)), np.zeros((B, K))
    for b in range(B):
        pb, yb = p[b][inl[b]], np.asarray(y[b])[inl[b]]
        sp[b] = pb.sum(axis=0)
        for c in range(K):
            tp[b, c] = pb[yb == c, c].sum()
            cnt[b, c] = float((yb == c).sum())
    return tp, sp, cnt


def coefficients(tp, sp, cnt, lam, alpha, beta, smooth):
    """-> dict(T [B, K], g_in [B, K], g_out [B, K], patch_loss [B], n [B]) from the soft counts; a patch with no pixel in the loss has
    T = 1, zero coefficients and no loss"""
    K = tp.shape[1]
    n = cnt.sum(axis=1)
    D = tp + alpha * (sp - tp) + beta * (cnt - tp) + smooth
    T = (tp + smooth) / D
    f = (lam * n / K)[:, None]
    g_in = -f * (D - (tp + smooth) * (1.0 - beta)) / (D * D)
    g_out = f * alpha * (tp + smooth) / (D * D)
    g_in[n == 0] = 0.0
    g_out[n == 0] = 0.0
    return dict(T=T, g_in=g_in, g_out=g_out, patch_loss=n * (lam / K) * (1.0 - T).sum(axis=1), n=n)


def dice(lg, y, K, lam, alpha=0.5, beta=0.5, smooth=1.0, loss_mask=None, inv_n=None):
    """lg [B, n, K] fp64 logits, y [B, n] labels, loss_mask [B, n] or None, inv_n the step's 1 / global pixels in the loss (default:
    1 / the in-loss pixels of this batch).  -> dict with the counts, the coefficients, loss (a float: inv_n sum_b patch_loss) and
    grad [B, n, K] = dL_dice / dlogits (exact zeros outside the loss)"""
    lg = np.asarray(lg, dtype=np.float64)
    y = np.asarray(y)
    inl = in_loss(y, K, loss_mask)
    if inv_n is None:
        inv_n = 1.0 / max(1, int(inl.sum()))
    p = softmax(lg.reshape(-1, K)).reshape(lg.shape)
    tp, sp, cnt = stats(p, y, inl, K)
    out = coefficients(tp, sp, cnt, lam, alpha, beta, smooth)
    onehot = np.minimum(y, K - 1)[..., None] == np.arange(K)
    g = np.where(onehot, out["g_in"][:, None, :], out["g_out"][:, None, :])
    grad = inv_n * p * (g - (p * g).sum(axis=2, keepdims=True))
    grad[~inl] = 0.0
    out.update(tp=tp, sp=sp, cnt=cnt, p=p, inl=inl, loss=float(inv_n * out["patch_loss"].sum()), grad=grad, inv_n=inv_n)
    return out
