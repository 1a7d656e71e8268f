"""The Lovasz-softmax term of the training loss (include/drs.h, "Training level: Lovasz-softmax term") stated in numpy:
the error keys, the order of every (patch, class), the Jaccard increments from exact integers, the per-(pixel, class) map the fused
classifier reads, the loss and the closed-form logit gradient.  tests/test_lovasz_plan.py holds it against fp64 autograd of the
paper's Algorithm 1 (Berman, Triki, Blaschko, CVPR 2018) written with torch.sort / cumsum.

Per patch b, over its n_b in-loss pixels only (loss_mask set where given, label < K):
    e_c   = 1 - p_c (as the sum of the other classes' terms) at a pixel with y = c, p_c elsewhere
    N_c   = #{y = c}; c is present when N_c > 0; C_b = the number of present classes
    order = e_c descending, ties towards the lower pixel index; at 0-based position r: F / Bg = foreground / background pixels before
            it, U = N_c + Bg, I = N_c - F
    dJ    = 1 / U (foreground), I / (U (U + 1)) (background)
    Loss_bc = sum_r e_(r) dJ_r        L_lov = inv_n sum_b (lam n_b / C_b) sum_{c present} Loss_bc
    g_c(p) = (lam n_b / C_b) (y_p == c ? -dJ : +dJ)        dL_lov / dlogit_k = inv_n P_k (g_k - sum_c P_c g_c)
"""
import numpy as np


def in_loss(y, K, loss_mask=None):
    """what "in the loss" means for the cross-entropy: loss_mask set when given, and label < K.  y, loss_mask: [B, n]"""
    y = np.asarray(y)
    ok = y < K
    return ok if loss_mask is None else ok & (np.asarray(loss_mask) != 0)


def error_keys(lg, y, K, loss_mask=None, dtype=np.float32):
    """lg [B, n, K] logits, y [B, n] -> the keys [B, n, K] in `dtype` arithmetic (float32: the kernel's formula, operation for
    operation; float64: the reference's), +0 at pixels that are not in the loss"""
    lg = np.asarray(lg, dtype=dtype)
    y = np.asarray(y)
    inl = in_loss(y, K, loss_mask)
    ex = np.exp(lg - lg.max(axis=2, keepdims=True)).astype(dtype)
    se = np.zeros(lg.shape[:2], dtype=dtype)
    for k in range(K):
        se = (se + ex[..., k]).astype(dtype)
    e = np.zeros(lg.shape, dtype=dtype)
    for c in range(K):
        so = np.zeros(lg.shape[:2], dtype=dtype)
        for k in range(K):
            if k != c:
                so = (so + ex[..., k]).astype(dtype)
        e[..., c] = (np.where(y == c, so, ex[..., c]) / se).astype(dtype)
    e[~inl] = 0
    return e


def order(e, inl):
    """e [n] keys, inl [n] bool -> the indices of the in-loss pixels by key descending, ties towards the lower index"""
    idx = np.flatnonzero(inl)
    return idx[np.argsort(-np.asarray(e, dtype=np.float64)[idx], kind="stable")]


def increments(fg):
    """fg [m] bool in sorted order (at least one set) -> (dJ [m] float64, F [m], U [m]) from exact integers"""
    fg = np.asarray(fg, dtype=bool)
    N = int(fg.sum())
    r = np.arange(fg.size, dtype=np.int64)
    F = np.cumsum(fg) - fg
    U = N + (r - F)
    I = N - F
    dJ = np.where(fg, 1.0 / U.astype(np.float64), I.astype(np.float64) / (U.astype(np.float64) * (U + 1).astype(np.float64)))
    return dJ, F, U


def from_keys(err, y, K, lam, loss_mask=None, values=None):
    """err [B, n, K] keys that give the ORDER (any float type), y [B, n], `values` [B, n, K] float64 the errors that enter the loss
    (default: err itself as float64).  -> dict(rank [B, n, K] int64, -1 where not in the loss or absent; g [B, n, K] float64;
    cls_loss [B, K]; patch_loss [B] = (lam n_b / C_b) sum_c Loss_bc; n [B]; C [B]; present [B, K]; factor [B])"""
    err = np.asarray(err)
    y = np.asarray(y)
    val = err.astype(np.float64) if values is None else np.asarray(values, dtype=np.float64)
    B, n, _ = err.shape
    inl = in_loss(y, K, loss_mask)
    rank = np.full((B, n, K), -1, dtype=np.int64)
    g = np.zeros((B, n, K))
    cls_loss = np.zeros((B, K))
    present = np.zeros((B, K), dtype=bool)
    nb = inl.sum(axis=1).astype(np.int64)
    C = np.zeros(B, dtype=np.int64)
    factor = np.zeros(B)
    for b in range(B):
        for c in range(K):
            present[b, c] = bool(((y[b] == c) & inl[b]).any())
        C[b] = int(present[b].sum())
        if nb[b] == 0:
            continue
        factor[b] = (lam * float(nb[b])) / float(C[b])
        for c in range(K):
            if not present[b, c]:
                continue
            o = order(err[b, :, c], inl[b])
            fg = y[b][o] == c
            dJ, _, _ = increments(fg)
            rank[b, o, c] = np.arange(o.size)
            g[b, o, c] = factor[b] * np.where(fg, -dJ, dJ)
            cls_loss[b, c] = float(np.sum(val[b, o, c] * dJ))
    patch_loss = factor * cls_loss.sum(axis=1)
    return dict(rank=rank, g=g, cls_loss=cls_loss, patch_loss=patch_loss, n=nb, C=C, present=present, factor=factor, inl=inl)


def softmax(lg):
    lg = np.asarray(lg, dtype=np.float64)
    e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def lovasz(lg, y, K, lam, loss_mask=None, inv_n=None, order_keys=None):
    """lg [B, n, K] logits (evaluated in fp64), y [B, n], loss_mask [B, n] or None, inv_n the step's 1 / global pixels in the loss
    (default: 1 / the in-loss pixels of this batch); order_keys [B, n, K] or None: keys to take the ORDER from (a device's own fp32
    keys) instead of the fp64 ones.  -> the dict of from_keys plus err (fp64 keys), p, loss (a float: inv_n sum_b patch_loss) and grad
    [B, n, K] = dL_lov / dlogits (exact zeros outside the loss)"""
    lg = np.asarray(lg, dtype=np.float64)
    y = np.asarray(y)
    err = error_keys(lg, y, K, loss_mask, dtype=np.float64)
    out = from_keys(err if order_keys is None else order_keys, y, K, lam, loss_mask, values=err)
    inl = out["inl"]
    if inv_n is None:
        inv_n = 1.0 / max(1, int(inl.sum()))
    p = softmax(lg)
    grad = inv_n * p * (out["g"] - (p * out["g"]).sum(axis=2, keepdims=True))
    grad[~inl] = 0.0
    out.update(err=err, p=p, loss=float(inv_n * out["patch_loss"].sum()), grad=grad, inv_n=inv_n)
    return out
