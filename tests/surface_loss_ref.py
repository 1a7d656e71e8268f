"""The boundary (surface) loss of the training loss (include/drs.h, "Training level: boundary (surface) loss") stated in
numpy: the counted pixels, the site sets, the exact signed squared distances, the per-(pixel, class) map the fused classifier reads,
the loss and the closed-form logit gradient.  tests/test_surface_loss_plan.py holds it against scipy's distance_transform_edt through
the published formula (Kervadec et al., MIDL 2019: edt(~pos) ~pos - (edt(pos) - 1) pos), against a brute-force minimum over all pairs,
and against fp64 autograd of sum softmax phi.

Per patch b, independent of other patches:
    counted = label < K, loss_mask set where given, valid set where given
    A_c = counted pixels with y = c, O_c = counted pixels with y != c; either empty: phi_c = 0 in the patch
    at p in O_c: D2 = min_{q in A_c} |p - q|^2, phi = +sqrt(D2);  at p in A_c: D2 = min_{q in O_c} |p - q|^2, phi = 1 - sqrt(D2)
    g_c(p) = (float)(lam clamp(phi, -clip, +clip))  (fp64, one rounding)        L_surf = inv_n sum_b sum_p sum_c g_c(p) P_c(p)
    dL_surf / dlogit_k = inv_n P_k (g_k - sum_c P_c g_c)
"""
import numpy as np

NONE = np.int64(1) << 40          # "no site": larger than any squared distance of a patch


def counted(y, K, loss_mask=None, valid=None):
    """y [B, S, S] labels -> bool [B, S, S]: label < K, loss_mask set where given, valid set where given"""
    y = np.asarray(y)
    ok = y < K
    if loss_mask is not None:
        ok = ok & (np.asarray(loss_mask) != 0)
    if valid is not None:
        ok = ok & (np.asarray(valid) != 0)
    return ok


def sq_dist_to(sites):
    """sites [S, S] bool (at least one set) -> int64 [S, S]: the exact squared Euclidean distance of every pixel to the nearest site.
    Two separable passes: the distance along the column to the nearest site of the column, then the minimum over the row of
    (x - i)^2 + column distance^2."""
    sites = np.asarray(sites, dtype=bool)
    S = sites.shape[0]
    r = np.arange(S, dtype=np.int64)
    dy2 = (r[:, None] - r[None, :]) ** 2                                     # [y, y']
    col = np.where(sites[None, :, :], dy2[:, :, None], NONE).min(axis=1)     # [y, x]: min over y' of (y - y')^2 at sites (y', x)
    return (dy2[None, :, :] + col[:, None, :]).min(axis=2)                   # [y, x]: min over i of (x - i)^2 + col[y, i]


def signed_sq_dist(y, K, loss_mask=None, valid=None):
    """y [B, S, S] -> phi2 int64 [B, S, S, K]: +D2 at counted pixels outside the class, -D2 at counted pixels of the class, 0 where
    the class has no distance map in the patch (a site set is empty) or the pixel is not counted"""
    y = np.asarray(y)
    cnt = counted(y, K, loss_mask, valid)
    B, S, _ = y.shape
    out = np.zeros((B, S, S, K), dtype=np.int64)
    for b in range(B):
        for c in range(K):
            A = cnt[b] & (y[b] == c)
            O = cnt[b] & (y[b] != c)
            if not A.any() or not O.any():
                continue
            out[b, :, :, c] = np.where(O, sq_dist_to(A), 0) - np.where(A, sq_dist_to(O), 0)
    return out


def phi_of(phi2):
    """phi2 (signed squared distances) -> phi float64: +sqrt(D2) outside, 1 - sqrt(D2) inside (the published -(sqrt(D2) - 1); +0 where
    D2 = 1), +0 where phi2 = 0"""
    phi2 = np.asarray(phi2, dtype=np.int64)
    sq = np.sqrt(np.abs(phi2).astype(np.float64))
    return np.where(phi2 < 0, 1.0 - sq, sq)


def grad_map(phi2, lam, clip=0.0):
    """-> (g64 float64: lam clamp(phi, -clip, +clip), g32 float32: that rounded once)"""
    phi = phi_of(phi2)
    if clip:
        phi = np.clip(phi, -float(clip), float(clip))
    g64 = float(lam) * phi
    return g64, g64.astype(np.float32)


def softmax(lg):
    lg = np.asarray(lg, dtype=np.float64)
    e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def surface_loss(lg, y, K, lam, clip=0.0, loss_mask=None, valid=None, inv_n=None):
    """lg [B, S, S, K] logits (evaluated in fp64), y [B, S, S]; inv_n the step's 1 / global pixels in the loss (default: 1 / the pixels
    of this batch with label < K and loss_mask set).  -> dict(phi2, phi, g (float64), g32, counted, p, patch_loss [B] = sum_p sum_c
    g32_c(p) P_c(p), abs_sum [B] = sum |g32 P| (what the term cancels from), loss = inv_n sum_b patch_loss, grad [B, S, S, K] =
    dL_surf / dlogits with the float32 map, inv_n)"""
    y = np.asarray(y)
    phi2 = signed_sq_dist(y, K, loss_mask, valid)
    g64, g32 = grad_map(phi2, lam, clip)
    cnt = counted(y, K, loss_mask, valid)
    p = softmax(lg)
    g = g32.astype(np.float64)
    terms = g * p * cnt[..., None]
    patch_loss = terms.reshape(y.shape[0], -1).sum(axis=1)
    abs_sum = np.abs(terms).reshape(y.shape[0], -1).sum(axis=1)
    if inv_n is None:
        inv_n = 1.0 / max(1, int(counted(y, K, loss_mask, None).sum()))
    grad = inv_n * p * (g - (p * g).sum(axis=-1, keepdims=True))
    grad[~cnt] = 0.0
    return dict(phi2=phi2, phi=phi_of(phi2), g=g64, g32=g32, counted=cnt, p=p, patch_loss=patch_loss, abs_sum=abs_sum,
                loss=float(inv_n * patch_loss.sum()), grad=grad, inv_n=inv_n)
