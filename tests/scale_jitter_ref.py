"""The numpy statement of the scale-jitter crop (include/drs.h above drs_crop_normalize_scaled), in the header's operation
order, in fp64: what tests/test_scale_jitter_plan.py holds to scipy and tests/test_gpu_scale_jitter.py holds the kernel to."""
import numpy as np


def centre(r, S, s, n):
    """one axis of the centre rule: c = r + S / 2 (r after the shift-back for side S), clamped to [a, n - a] with a = S / (2 s) when
    2 a <= n, else n / 2"""
    c = float(r) + float(S) / 2.0
    a = float(S) / (2.0 * float(s))
    if 2.0 * a <= float(n):
        return min(max(c, a), float(n) - a)
    return float(n) / 2.0


def geometry(r, c, S, s, h, w):
    """(step, cy, cx) of the side-S patch at (r, c) -- before the shift-back -- of an h x w map at scale s"""
    r, c = min(int(r), h - S), min(int(c), w - S)              # isprs:260-269
    return 1.0 / float(s), centre(r, S, s, h), centre(c, S, s, w)


def axis(S, c, step, n):
    """per patch pixel index p of one axis: (u, valid, i0, i1, l, label index)"""
    p = np.arange(S, dtype=np.float64)
    t = (p + 0.5) - 0.5 * float(S)
    u = c + t * step
    valid = (u >= 0.0) & (u <= float(n))
    src = np.minimum(np.maximum(u - 0.5, 0.0), float(n - 1))
    i0 = np.floor(src).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    il = np.minimum(np.floor(np.where(valid, u, 0.0)).astype(np.int64), n - 1)
    return u, valid, i0, i1, src - i0, il


def resample_geo(x, lab, S, geo):
    """the S x S patch of the footprint geo = (step, cy, cx) of the map x [h][w][C] (taken to fp64) with labels lab [h][w]:
    (patch fp64 [S][S][C], labels [S][S] of lab's dtype, valid bool [S][S]); invalid pixels are value 0, label 0"""
    x = np.asarray(x, dtype=np.float64)
    lab = np.asarray(lab)
    h, w = x.shape[:2]
    step, cy, cx = (float(v) for v in geo)
    _, vy, y0, y1, ly, yl = axis(S, cy, step, h)
    _, vx, x0, x1, lx, xl = axis(S, cx, step, w)
    ly, lx = ly.reshape(S, 1, 1), lx.reshape(1, S, 1)
    r0, r1 = x[y0], x[y1]
    patch = (1.0 - ly) * ((1.0 - lx) * r0[:, x0] + lx * r0[:, x1]) + ly * ((1.0 - lx) * r1[:, x0] + lx * r1[:, x1])
    valid = vy.reshape(S, 1) & vx.reshape(1, S)
    patch = np.where(valid[:, :, None], patch, 0.0)
    labels = np.where(valid, lab[yl][:, xl], 0).astype(lab.dtype)
    return patch, labels, valid


def resample(x, lab, r, c, S, s):
    """the patch of side S at (r, c) of the map x with labels lab at scale s: resample_geo of geometry"""
    return resample_geo(x, lab, S, geometry(r, c, S, s, x.shape[0], x.shape[1]))
