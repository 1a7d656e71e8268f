"""The numpy statement of the boundary weight map and of the boundary-weighted training loss (include/drs.h "Training level",
DESIGN.md 3c) that the tests hold the kernels to: brute force over the window, integers for the distance, fp64 for the weight.
tests/test_boundary_weight_plan.py checks it against hand-worked maps; tests/test_gpu_boundary_weight.py uses it on the device.

Rule: for a valid pixel p of a patch, D2(p) = min dy^2 + dx^2 over q = p + (dy, dx) with |dy|, |dx| <= R, q inside the same patch,
q valid and lab[q] != lab[p]; infinite if there is none or if p is invalid.  w = 1 where D2 is infinite, else 1 + a exp(-D2 c)."""
import numpy as np

from focal_ref import focal_closed_form

INF = np.iinfo(np.int64).max


def boundary_d2(lab, valid, R):
    """lab uint8 [B][S][S], valid the same shape or None, R >= 1 -> int64 [B][S][S], INF where D2 is infinite.  Every offset of the
    window is tried for every pixel: no separability, no early exit."""
    lab = np.asarray(lab)
    B, S, _ = lab.shape
    ok = np.ones(lab.shape, dtype=bool) if valid is None else np.asarray(valid) != 0
    d2 = np.full(lab.shape, INF, dtype=np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if (dy == 0 and dx == 0) or abs(dy) >= S or abs(dx) >= S:
                continue
            # p ranges over the pixels whose q = p + (dy, dx) lies inside the patch
            py = slice(max(0, -dy), min(S, S - dy))
            px = slice(max(0, -dx), min(S, S - dx))
            qy = slice(max(0, dy), min(S, S + dy))
            qx = slice(max(0, dx), min(S, S + dx))
            hit = ok[:, py, px] & ok[:, qy, qx] & (lab[:, py, px] != lab[:, qy, qx])
            view = d2[:, py, px]
            view[hit] = np.minimum(view[hit], dy * dy + dx * dx)
    return d2


def boundary_d2_loops(lab, valid, R):
    """the same rule as four nested loops, for the small hand-worked maps: the statement boundary_d2 is itself checked against"""
    lab = np.asarray(lab)
    B, S, _ = lab.shape
    d2 = np.full(lab.shape, INF, dtype=np.int64)
    for b in range(B):
        for y in range(S):
            for x in range(S):
                if valid is not None and not valid[b, y, x]:
                    continue
                for qy in range(max(0, y - R), min(S, y + R + 1)):
                    for qx in range(max(0, x - R), min(S, x + R + 1)):
                        if (valid is None or valid[b, qy, qx]) and lab[b, qy, qx] != lab[b, y, x]:
                            d2[b, y, x] = min(d2[b, y, x], (qy - y) ** 2 + (qx - x) ** 2)
    return d2


def boundary_weight(lab, valid, R, a, c):
    """-> (weight float64 [B][S][S], d2 int64 with INF): the weight BEFORE its one rounding to float32"""
    d2 = boundary_d2(lab, valid, R)
    fin = d2 != INF
    w = np.ones(d2.shape, dtype=np.float64)
    w[fin] = 1.0 + float(a) * np.exp(-d2[fin].astype(np.float64) * float(c))
    return w, d2


def d2_u16(d2):
    """what drs_patch_boundary_weight stores: min(D2, 65535) as uint16"""
    return np.minimum(d2, 65535).astype(np.uint16)


def pixel_weighted_closed_form(logits, y, wc, gamma, pw):
    """focal_closed_form with the per-pixel weight pw [M] multiplied into the loss term and the logit gradient; nothing else changes.
    Returns its dict with term and grad replaced (no normaliser applied)."""
    ref = dict(focal_closed_form(logits, y, wc, gamma))
    pw = np.asarray(pw, dtype=np.float64)
    ref["term"] = ref["term"] * pw
    ref["grad"] = ref["grad"] * pw[:, None]
    return ref
