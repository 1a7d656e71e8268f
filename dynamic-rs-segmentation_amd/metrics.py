"""Scores derived from a K x K confusion matrix (rows = label, cols = prediction).

The reference computes them partly by hand (isprs:526-529, 1298-1303, 1601-1605) and partly with sklearn on the
flattened label/prediction arrays (cohen_kappa_score, f1_score: isprs:1305-1310, 1607-1608); all of them are
functions of the confusion matrix, which is what the device produces.
"""
import numpy as np


def overall_and_normalized(cm):
    """(#correct, overall accuracy, class-normalised accuracy): mean of per-class recalls, classes without
    pixels contribute 0 and the divisor is always K (isprs:526-529)."""
    cm = np.asarray(cm, dtype=np.float64)
    rows = cm.sum(axis=1)
    rec = np.where(rows != 0, np.diag(cm) / np.where(rows != 0, rows, 1), 0.0)
    tot = cm.sum()
    return int(np.trace(cm)), (np.trace(cm) / tot if tot else 0.0), float(rec.sum() / cm.shape[0])


def f1_per_class(cm):
    """sklearn f1_score(average=None) over the labels present in y_true or y_pred."""
    cm = np.asarray(cm, dtype=np.float64)
    tp = np.diag(cm)
    fp = cm.sum(axis=0) - tp
    fn = cm.sum(axis=1) - tp
    present = (cm.sum(axis=0) + cm.sum(axis=1)) > 0
    den = 2 * tp + fp + fn
    f1 = np.where(den > 0, 2 * tp / np.where(den > 0, den, 1), 0.0)
    return f1[present], present


def f1_macro(cm):
    f1, _ = f1_per_class(cm)
    return float(f1.mean()) if len(f1) else 0.0


def iou_per_class(cm):
    """(intersection over union of the classes present in the labels or the predictions, the presence mask): tp / (tp + fp + fn), the
    presence rule of f1_per_class."""
    cm = np.asarray(cm, dtype=np.float64)
    tp = np.diag(cm)
    union = cm.sum(axis=0) + cm.sum(axis=1) - tp
    present = union > 0
    return tp[present] / union[present], present


def mean_iou(cm):
    iou, _ = iou_per_class(cm)
    return float(iou.mean()) if len(iou) else 0.0


def boundary_scores(hist, distances):
    """Boundary-quality scores from the table of drs_boundary_histogram (include/drs.h): hist [(n+1)][(n+1)][K][K]
    integers, hist[bg][bp][t][p] = the counted pixels of truth class t predicted p whose distance bin is bg in the truth map and bp
    in the prediction (bin i: within distances[i] of a pixel that carries another byte and not within distances[i - 1]; bin n:
    further than the last).  Everything below is a sum over the table:
      CM = sum over bg, bp                                  the plain confusion matrix (what drs_confusion gives)
      trimap of d_i (Kohli et al. 2009)    T_i = sum over bg <= i and every bp: its pixel count, overall_and_normalized(T_i)
      Boundary IoU of d_i and class c (Cheng et al. 2021)   I / (G + P - I) with I = sum over bg <= i, bp <= i of hist[bg][bp][c][c],
          G = sum over bg <= i, every bp, every j of hist[bg][bp][c][j],  P = sum over bp <= i, every bg, every j of hist[bg][bp][j][c];
          a class with G + P - I = 0 is absent, the mean is over the present classes (0.0 without any), as f1_per_class
    Returns {"distances", "confusion", "iou_per_class" (K values, 0 for an absent class), "mean_iou", "bands": [{"d", "count",
    "accuracy", "normalized_accuracy", "confusion", "boundary_iou_per_class" (K values, 0 for an absent class),
    "boundary_iou_present", "boundary_iou"} per distance]}.  A table of another shape, of a non-integer dtype or with a negative
    entry raises ValueError."""
    h = np.asarray(hist)
    n = len(distances)
    if (h.ndim != 4 or h.shape[0] != n + 1 or h.shape[1] != n + 1 or h.shape[2] != h.shape[3] or h.shape[2] < 1
            or not np.issubdtype(h.dtype, np.integer) or np.any(h < 0)):
        raise ValueError("boundary table: expected [%d][%d][K][K] non-negative integers for the distances %r, not %s of shape %r"
                         % (n + 1, n + 1, tuple(distances), h.dtype, h.shape))
    h = h.astype(np.int64)
    K = h.shape[2]
    cm = h.sum(axis=(0, 1))
    iou_full = np.zeros(K, dtype=np.float64)
    iou, present = iou_per_class(cm)
    iou_full[present] = iou
    bands = []
    for i, d in enumerate(distances):
        t = h[:i + 1].sum(axis=(0, 1))
        _, oa, na = overall_and_normalized(t)
        inter = np.diagonal(h[:i + 1, :i + 1].sum(axis=(0, 1))).astype(np.float64)
        g = h[:i + 1].sum(axis=(0, 1, 3)).astype(np.float64)
        p = h[:, :i + 1].sum(axis=(0, 1, 2)).astype(np.float64)
        union = g + p - inter
        there = union > 0
        biou = np.where(there, inter / np.where(there, union, 1.0), 0.0)
        bands.append({"d": int(d), "count": int(t.sum()), "accuracy": float(oa), "normalized_accuracy": float(na), "confusion": t,
                      "boundary_iou_per_class": biou, "boundary_iou_present": there,
                      "boundary_iou": float(biou[there].mean()) if there.any() else 0.0})
    return {"distances": tuple(int(d) for d in distances), "confusion": cm, "iou_per_class": iou_full, "mean_iou": mean_iou(cm),
            "bands": bands}


def object_scores(table):
    """Object-level scores from the table of drs_object_table (include/drs.h): table [K][4][32] integers, by
    floor(log2(size)): row 0 truth objects, row 1 predicted objects, row 2 matched truth objects, row 3 the sum over them of
    floor(IoU 2^20).  Per class, in fp64:  TP = sum of row 2, FN = sum of row 0 - TP, FP = sum of row 1 - TP;
      precision = TP / (TP + FP), recall = TP / (TP + FN), RQ = F1 = 2 TP / (2 TP + FP + FN)      (recognition quality)
      SQ = sum of row 3 / (TP 2^20)    the mean IoU of the matched objects                        (segmentation quality)
      PQ = SQ RQ                       (Kirillov et al. 2019)
    A class with no truth object and no predicted object is absent: it has no score (nan) and is left out of the means, the way
    iou_per_class treats an absent class.  Of a present class, precision is nan without a predicted object, recall without a truth
    object and SQ without a match (PQ is then 0, as its sum form says); a mean runs over the classes that have the score, 0.0 without
    any.  Returns {"truth", "predicted", "matched" (K ints each), "present", "precision", "recall", "f1", "sq", "pq" (K values),
    "recall_by_size" ([K][32], nan where no truth object has that size), "mean_precision", "mean_recall", "mean_f1", "mean_sq",
    "mean_pq", "all": the same counts and scores of the table summed over the classes}.  A table of another shape, of a non-integer
    dtype, with a negative entry or with more matches than objects raises ValueError."""
    t = np.asarray(table)
    if t.ndim != 3 or t.shape[0] < 1 or t.shape[1:] != (4, 32) or not np.issubdtype(t.dtype, np.integer) or np.any(t < 0):
        raise ValueError("object table: expected [K][4][32] non-negative integers, not %s of shape %r" % (t.dtype, t.shape))
    t = t.astype(np.int64)
    if np.any(t[:, 2] > t[:, 0]) or np.any(t[:, 2].sum(axis=1) > t[:, 1].sum(axis=1)):
        raise ValueError("object table: more matched objects than objects")

    def scores(rows):
        """rows [..][4][32] -> the counts and scores along the leading axes"""
        nt, npred, tp, s3 = [rows[..., r, :].sum(axis=-1) for r in range(4)]
        fn, fp = nt - tp, npred - tp
        present = (nt + npred) > 0
        nan = np.full(nt.shape, np.nan)
        div = lambda a, b, where: np.where(where, a / np.where(where, b, 1), nan)
        f1 = div(2.0 * tp, 2.0 * tp + fp + fn, present)
        sq = div(s3 / 2.0 ** 20, tp, tp > 0)
        return {"truth": nt, "predicted": npred, "matched": tp, "present": present, "precision": div(tp, npred, npred > 0),
                "recall": div(tp, nt, nt > 0), "f1": f1, "sq": sq, "pq": np.where(tp > 0, sq * f1, np.where(present, 0.0, np.nan))}
    out = scores(t)
    out["recall_by_size"] = np.where(t[:, 0] > 0, t[:, 2] / np.where(t[:, 0] > 0, t[:, 0], 1), np.nan)
    for key in ("precision", "recall", "f1", "sq", "pq"):
        have = ~np.isnan(out[key])
        out["mean_" + key] = float(out[key][have].mean()) if have.any() else 0.0
    whole = scores(t.sum(axis=0))
    out["all"] = {k: (bool(v) if k == "present" else int(v) if k in ("truth", "predicted", "matched") else float(v)) for k, v in whole.items()}
    return out


SURFACE_BINS = 4096          # DRS_SURFACE_BINS of include/drs.h: quarter-pixel bins, the last one open


def surface_scores(table, tolerances):
    """Surface-distance scores from the table of drs_surface_histogram (include/drs.h): table [2][K][BINS + 2]
    integers; direction 0 walks the contour pixels of a class in the truth with their distance d to the class's contour in the
    prediction, direction 1 the reverse.  Of [dir][c]: entry b < BINS counts the pixels with ceil(4 d) = b (the last bin: everything
    from (BINS - 1) / 4 pixels on), entry BINS is the sum of floor(1024 d), entry BINS + 1 the pixels whose counterpart contour is
    empty (unsited).  Per class, in fp64, with n_dir the sited pixels of a direction:
      assd   = (sum_0 + sum_1) / 1024 / (n_0 + n_1)                  average symmetric surface distance, in pixels
      hd95   = max over the directions of b / 4, b the bin that holds the ceil(0.95 n_dir)-th smallest distance: the Hausdorff
               distance at the 95th percentile, rounded UP to a quarter pixel; nan when either direction has no sited pixel;
               `saturated` says that b is the last bin: the value is then a lower bound
      hd100  = likewise with the largest distance
      nsd[i] = (pixels of both directions with b <= 4 tolerances[i]) / (all walked pixels of both directions, unsited included): the
               normalised surface Dice at that tolerance, exact for integer tolerances
    A score a class does not have is nan; a mean runs over the classes that have it (nan without any).  Returns {"tolerances",
    "n_truth", "n_pred" (the contour pixels, unsited included), "unsited_truth", "unsited_pred" (K ints each), "assd", "hd95", "hd100"
    (K values), "saturated" (K bools), "nsd" ([len(tolerances)][K]), "mean_assd", "mean_hd95", "mean_hd100", "mean_nsd" (one per
    tolerance)}.  A table of another shape, of a non-integer dtype or with a negative entry raises ValueError."""
    t = np.asarray(table)
    B = SURFACE_BINS
    if t.ndim != 3 or t.shape[0] != 2 or t.shape[1] < 1 or t.shape[2] != B + 2 or not np.issubdtype(t.dtype, np.integer) or np.any(t < 0):
        raise ValueError("surface table: expected [2][K][%d] non-negative integers, not %s of shape %r" % (B + 2, t.dtype, t.shape))
    t = t.astype(np.int64)
    K = t.shape[1]
    bins, fsum, unsited = t[:, :, :B], t[:, :, B], t[:, :, B + 1]
    cum = np.cumsum(bins, axis=2)
    n = cum[:, :, -1]                                                     # [2][K] sited pixels
    walked = n + unsited
    both = n.sum(axis=0)
    nan = np.full(K, np.nan)
    assd = np.where(both > 0, fsum.sum(axis=0) / 1024.0 / np.where(both > 0, both, 1), nan)

    def quantile_bin(rank):
        """[2][K]: the first bin whose cumulative count reaches rank (>= 1 where n > 0)"""
        return np.array([[int(np.searchsorted(cum[d, c], rank[d, c], side="left")) if n[d, c] > 0 else 0 for c in range(K)]
                         for d in range(2)])
    have = (n > 0).all(axis=0)
    b95, b100 = quantile_bin((95 * n + 99) // 100).max(axis=0), quantile_bin(n).max(axis=0)
    out = {"tolerances": tuple(int(v) for v in tolerances), "n_truth": walked[0], "n_pred": walked[1], "unsited_truth": unsited[0],
           "unsited_pred": unsited[1], "assd": assd, "hd95": np.where(have, b95 / 4.0, nan), "hd100": np.where(have, b100 / 4.0, nan),
           "saturated": have & (b95 == B - 1)}
    total = walked.sum(axis=0)
    out["nsd"] = np.array([np.where(total > 0, cum[:, :, min(4 * int(tol), B - 1)].sum(axis=0) / np.where(total > 0, total, 1), nan)
                           for tol in tolerances]).reshape(len(out["tolerances"]), K)
    mean = lambda v: float(v[~np.isnan(v)].mean()) if (~np.isnan(v)).any() else float("nan")
    for key in ("assd", "hd95", "hd100"):
        out["mean_" + key] = mean(out[key])
    out["mean_nsd"] = [mean(row) for row in out["nsd"]]
    return out


def cohen_kappa(cm):
    """sklearn cohen_kappa_score(y_true, y_pred) from the confusion matrix."""
    cm = np.asarray(cm, dtype=np.float64)
    n = cm.sum()
    if n == 0:
        return 0.0
    po = np.trace(cm) / n
    pe = float((cm.sum(axis=0) * cm.sum(axis=1)).sum()) / (n * n)
    return float((po - pe) / (1 - pe)) if pe != 1 else 0.0


def calibration(hist, bins=15):
    """Calibration scores from a reliability table (drs_reliability_histogram): hist [256][2] integers, hist[c] = (pixels whose
    confidence byte is c, those of them predicted right).  The confidence of byte c is c / 255; the bins are `bins` equal-width
    intervals of [0, 1], bin b = [b / bins, (b + 1) / bins), the last one closed (byte c falls into min(c * bins // 255, bins - 1)).
    With n_b, conf_b, acc_b the pixel count, mean confidence and accuracy of bin b and N = sum n_b:
      ece = sum_b (n_b / N) |acc_b - conf_b|      (expected calibration error)
      mce = max over non-empty b of |acc_b - conf_b|
    Returns {"ece", "mce", "mean_confidence", "accuracy", "count", "bins": [{"lo", "hi", "count", "confidence", "accuracy"}, ...]};
    an empty table gives zeros (and zeros in the empty bins)."""
    h = np.asarray(hist)
    bins = int(bins)
    if h.shape != (256, 2) or not np.issubdtype(h.dtype, np.integer) or np.any(h < 0) or np.any(h[:, 1] > h[:, 0]):
        raise ValueError("reliability table: expected [256][2] non-negative integers with hist[c][1] <= hist[c][0]")
    if bins < 1:
        raise ValueError("calibration: bins must be >= 1, not %r" % bins)
    n = h[:, 0].astype(np.float64)
    right = h[:, 1].astype(np.float64)
    conf = np.arange(256, dtype=np.float64) / 255.0
    which = np.minimum(np.arange(256) * bins // 255, bins - 1)
    n_b = np.bincount(which, weights=n, minlength=bins)
    c_b = np.bincount(which, weights=n * conf, minlength=bins)
    r_b = np.bincount(which, weights=right, minlength=bins)
    total = float(n.sum())
    some = n_b > 0
    den = np.where(some, n_b, 1.0)
    conf_b, acc_b = np.where(some, c_b / den, 0.0), np.where(some, r_b / den, 0.0)
    gap = np.abs(acc_b - conf_b)
    table = [{"lo": b / float(bins), "hi": (b + 1) / float(bins), "count": int(n_b[b]), "confidence": float(conf_b[b]),
              "accuracy": float(acc_b[b])} for b in range(bins)]
    if total == 0:
        return {"ece": 0.0, "mce": 0.0, "mean_confidence": 0.0, "accuracy": 0.0, "count": 0, "bins": table}
    return {"ece": float((n_b / total * gap).sum()), "mce": float(gap[some].max()), "mean_confidence": float(c_b.sum() / total),
            "accuracy": float(r_b.sum() / total), "count": int(total), "bins": table}


def fit_temperature(stats_fn, lo=1.0 / 64.0, hi=64.0, max_iter=60):
    """Temperature scaling (Guo et al., On calibration of modern neural networks): the inverse temperature beta = 1 / T
    in [lo, hi] that minimises the negative log-likelihood L(beta) of softmax(beta u) on labelled pixels.  stats_fn(beta) returns the
    sufficient statistics (N, L, G, H, A) of include/drs.h's drs_temperature_stats: the count, L, dL/dbeta, d2L/dbeta2 >= 0 and
    sum |mu - u_y|, the scale G is judged against.  L is convex in beta, so this is a safeguarded Newton iteration on G = 0:
      - G(lo) >= 0 returns lo and G(hi) <= 0 returns hi, both with at_bound (perfectly separable data ends at hi);
      - otherwise, from beta = 1: stop when |G| <= 1e-12 A; else shrink the bracket (hi = beta if G > 0, else lo = beta), propose
        beta - G / H, take sqrt(lo hi) instead if H <= 0 or the proposal leaves the open bracket, and stop when the step is
        <= 1e-14 beta.  The value returned is the last beta evaluated, so nll_after is its L / N.
      - N = 0, or A = 0 and H = 0 at lo (one class, or every score vector constant: L does not depend on beta), returns beta = 1 with
        degenerate.
    At most 2 + max_iter evaluations.  Returns {"beta", "temperature", "nll_before" (L / N at beta = 1), "nll_after", "count",
    "iterations" (evaluations made), "at_bound", "degenerate"}."""
    lo, hi, max_iter = float(lo), float(hi), int(max_iter)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= 1.0 <= hi) or max_iter < 1:
        raise ValueError("fit_temperature: expected finite 0 < lo <= 1 <= hi and max_iter >= 1, not lo=%r hi=%r max_iter=%r" % (lo, hi, max_iter))
    evals = [0]

    def stats(beta):
        evals[0] += 1
        N, L, G, H, A = (float(x) for x in stats_fn(beta))
        return N, L, G, H, A

    def result(beta, before, after, N, at_bound=False, degenerate=False):
        return {"beta": beta, "temperature": 1.0 / beta, "nll_before": before, "nll_after": after, "count": int(N),
                "iterations": evals[0], "at_bound": at_bound, "degenerate": degenerate}
    N, L_lo, G_lo, H_lo, A_lo = stats(lo)
    if N == 0:
        return result(1.0, 0.0, 0.0, 0, degenerate=True)
    if A_lo == 0.0 and H_lo == 0.0:
        return result(1.0, L_lo / N, L_lo / N, N, degenerate=True)
    _, L_hi, G_hi, _, _ = stats(hi)
    if G_lo >= 0.0 or G_hi <= 0.0:
        beta, L_b = (lo, L_lo) if G_lo >= 0.0 else (hi, L_hi)
        before = L_b / N if beta == 1.0 else stats(1.0)[1] / N
        return result(beta, before, L_b / N, N, at_bound=True)
    new, before = 1.0, None
    for _ in range(max_iter):
        beta = new
        _, L, G, H, A = stats(beta)
        before = L / N if before is None else before
        if abs(G) <= 1e-12 * A:
            break
        if G > 0.0:
            hi = beta
        else:
            lo = beta
        new = beta - G / H if H > 0.0 else lo
        if not lo < new < hi:
            new = float(np.sqrt(lo * hi))
        if abs(new - beta) <= 1e-14 * beta:
            break
    return result(beta, before, L / N, N)
