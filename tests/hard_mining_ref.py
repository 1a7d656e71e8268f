"""Online hard example mining in the training loss (include/drs.h, "Training level: hard example mining") stated in
numpy: the keys, the kept count, the selection, the fp32 weight map, and the mined loss with its logit gradient in fp64.
tests/test_hard_mining_plan.py holds the gradient against fp64 autograd and finite differences.

For patch b, over the in-loss pixels of that patch alone (loss_mask set when given, label < K):
    n_b = their number            k_b = min(n_b, max(ceil(keep n_b), min_keep))       (float64 product and ceil)
    key = log(se) + (max - logit_y), the plain cross-entropy (>= +0)
    kept = the k_b largest keys, ties towards the lower pixel index: np.lexsort((index, -key))[:k_b]
    weight[p] = kept ? float32(float64(n_b) / float64(k_b)) * w_in[p] : 0       (one fp32 multiply; w_in = 1 without a map)
    loss = inv_n sum_b sum_p weight[p] term(p), the weights constants in the gradient
"""
import numpy as np


def in_loss(y, K, loss_mask=None):
    """what "in the loss" means for the cross-entropy: loss_mask set when given, and label < K.  y, loss_mask: [B, n]"""
    y = np.asarray(y)
    ok = y < K
    return ok if loss_mask is None else ok & (np.asarray(loss_mask) != 0)


def cross_entropy(lg, y):
    """lg [..., K] logits (evaluated in fp64), y [...] labels < K -> log(se) + (max - logit_y), the max-subtracted form"""
    lg = np.asarray(lg, dtype=np.float64)
    mx = lg.max(axis=-1)
    se = np.exp(lg - mx[..., None]).sum(axis=-1)
    ly = np.take_along_axis(lg, np.asarray(y, dtype=np.int64)[..., None], axis=-1)[..., 0]
    return np.log(se) + (mx - ly)


def kept_count(n, keep, min_keep):
    """k_b of a patch with n in-loss pixels"""
    n = int(n)
    return min(n, max(int(np.ceil(np.float64(keep) * np.float64(n))), int(min_keep)))


def select(keys, inl, keep, min_keep):
    """keys [B, n] (any float type; only in-loss entries are looked at), inl [B, n] bool -> (kept [B, n] bool, n_b [B], k_b [B])"""
    keys, inl = np.asarray(keys), np.asarray(inl, dtype=bool)
    B, n = keys.shape
    kept = np.zeros((B, n), dtype=bool)
    nb, kb = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        idx = np.flatnonzero(inl[b])
        nb[b] = idx.size
        kb[b] = kept_count(idx.size, keep, min_keep)
        order = np.lexsort((idx, -keys[b, idx].astype(np.float64)))        # largest key first, ties by the lower pixel index
        kept[b, idx[order[:kb[b]]]] = True
    return kept, nb, kb


def weights(keys, inl, keep, min_keep, w_in=None):
    """-> (weight float32 [B, n], k_b int [B]): exactly what drs_patch_hard_weight leaves for these keys"""
    kept, nb, kb = select(keys, inl, keep, min_keep)
    scale = np.ones(len(nb), dtype=np.float32)
    some = kb > 0
    scale[some] = (nb[some].astype(np.float64) / kb[some].astype(np.float64)).astype(np.float32)
    w = np.ones(kept.shape, dtype=np.float32) if w_in is None else np.asarray(w_in, dtype=np.float32).reshape(kept.shape)
    out = (scale[:, None] * w).astype(np.float32)                          # fp32 times fp32, rounded once
    out[~kept] = 0.0
    return out, kb


def mined(lg, y, K, keep, min_keep=0, loss_mask=None, inv_n=None, w_in=None):
    """lg [B, n, K] logits, y [B, n] labels, loss_mask [B, n] or None, inv_n the step's 1 / global pixels in the loss (default: 1 /
    the in-loss pixels of this batch), w_in [B, n] an incoming pixel map or None.  Everything in fp64 from the logits as given.  ->
    dict(ce [B, n] (0 outside the loss), inl, kept, n, k, weight float32 [B, n], loss = inv_n sum weight ce, grad [B, n, K] = dloss /
    dlogits with the selection held constant: inv_n weight (softmax - onehot))"""
    lg = np.asarray(lg, dtype=np.float64)
    y = np.asarray(y)
    inl = in_loss(y, K, loss_mask)
    if inv_n is None:
        inv_n = 1.0 / max(1, int(inl.sum()))
    yy = np.minimum(y, K - 1)
    ce = np.where(inl, cross_entropy(lg, yy), 0.0)
    kept, nb, kb = select(ce, inl, keep, min_keep)
    w, _ = weights(ce, inl, keep, min_keep, w_in)
    e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    onehot = (yy[..., None] == np.arange(K)).astype(np.float64)
    w64 = w.astype(np.float64)
    grad = inv_n * w64[..., None] * (p - onehot)
    return dict(ce=ce, inl=inl, kept=kept, n=nb, k=kb, weight=w, loss=float(inv_n * (w64 * ce).sum()), grad=grad, inv_n=inv_n)
