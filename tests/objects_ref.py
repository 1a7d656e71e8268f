"""The object match, the object table and the object scores of DESIGN.md 8a.9 / include/drs.h (drs_object_match, drs_object_table;
loops.object_table, metrics.object_scores) stated in numpy.  Integer arithmetic up to the scores; numpy only.

  counted      a truth pixel with truth != ignore_label and truth < K
  truth object a component (sieve_ref.components) of truth whose byte is counted; predicted object: a component of pred with byte < K
  cover(p)     the pixels of p whose truth pixel is counted;   I(t, p) = |t n p| for t, p of the same byte
  match        3 I > |t| + cover(p), i.e. I / (|t| + cover(p) - I) > 1/2; unique in both directions
  table        [K][4][32] by floor(log2(size)): truth objects; predicted objects (matched, or unmatched with 2 cover >= |p|); matched
               truth objects; sum over them of floor(I 2^20 / (|t| + cover(p) - I))"""
import numpy as np

import sieve_ref


def counted_mask(truth, K, ignore_label):
    truth = np.asarray(truth)
    return (truth != ignore_label) & (truth < K)


def match(truth, pred, K, ignore_label, connectivity):
    """(match int32 [h w], inter uint32 [h w], cover uint32 [h w], (tlabel, tsize, plabel, psize) flat int64) -- the full pair table
    of the two labellings by np.unique on (tlabel, plabel), the rule applied to every pair literally"""
    truth, pred = np.asarray(truth), np.asarray(pred)
    h, w = truth.shape
    n = h * w
    tl, ts = [a.reshape(-1).astype(np.int64) for a in sieve_ref.components(truth, connectivity)]
    pl, ps = [a.reshape(-1).astype(np.int64) for a in sieve_ref.components(pred, connectivity)]
    tf, pf = truth.reshape(-1).astype(np.int64), pred.reshape(-1).astype(np.int64)
    counted = counted_mask(tf, K, ignore_label)
    idx = np.arange(n)
    cover = np.zeros(n, dtype=np.int64)
    np.add.at(cover, pl[counted & (pf < K)], 1)
    out_match = np.full(n, -2, dtype=np.int64)
    out_match[(tl == idx) & counted] = -1
    out_inter = np.zeros(n, dtype=np.int64)
    same = counted & (pf == tf)
    pairs, counts = np.unique(np.stack([tl[same], pl[same]], axis=1), axis=0, return_counts=True) if same.any() else (np.zeros((0, 2), np.int64), [])
    for (t, p), I in zip(pairs, counts):
        if 3 * int(I) > int(ts[t]) + int(cover[p]):
            assert out_match[t] == -1 and not (out_match == p).any(), "the match is not unique"
            out_match[t] = p
            out_inter[t] = I
    return out_match.astype(np.int32), out_inter.astype(np.uint32), cover.astype(np.uint32), (tl, ts, pl, ps)


def table_from(truth, pred, K, ignore_label, m, inter, cover, labels):
    """table [K][4][32] int64 from the outputs of match"""
    tl, ts, pl, ps = labels
    tf, pf = np.asarray(truth).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    m, inter, cover = [np.asarray(a).reshape(-1).astype(np.int64) for a in (m, inter, cover)]
    n = tf.size
    idx = np.arange(n)
    table = np.zeros((K, 4, 32), dtype=np.int64)
    bin_of = lambda v: int(v).bit_length() - 1
    matched_p = set(int(v) for v in m[m >= 0])
    for t in idx[(tl == idx) & counted_mask(tf, K, ignore_label)]:
        b = bin_of(ts[t])
        table[tf[t], 0, b] += 1
        if m[t] >= 0:
            I, c = int(inter[t]), int(cover[m[t]])
            table[tf[t], 2, b] += 1
            table[tf[t], 3, b] += (I << 20) // (int(ts[t]) + c - I)
    for p in idx[(pl == idx) & (pf < K)]:
        if int(p) in matched_p or 2 * int(cover[p]) >= int(ps[p]):
            table[pf[p], 1, bin_of(ps[p])] += 1
    return table


def table(truth, pred, K, ignore_label, connectivity):
    m, inter, cover, labels = match(truth, pred, K, ignore_label, connectivity)
    return table_from(truth, pred, K, ignore_label, m, inter, cover, labels)


def branches(truth, pred, K, ignore_label, connectivity):
    """what a fixture exercises: {"matched", "unmatched_truth", "unmatched_pred" (counted false positives), "dropped_pred"}"""
    m, inter, cover, (tl, ts, pl, ps) = match(truth, pred, K, ignore_label, connectivity)
    idx = np.arange(m.size)
    proots = idx[(pl == idx) & (np.asarray(pred).reshape(-1) < K)]
    matched_p = set(int(v) for v in m[m >= 0])
    free = [p for p in proots if int(p) not in matched_p]
    kept = sum(1 for p in free if 2 * int(cover[p]) >= int(ps[p]))
    return {"matched": int((m >= 0).sum()), "unmatched_truth": int((m == -1).sum()), "unmatched_pred": kept, "dropped_pred": len(free) - kept}


def scores(tab):
    """metrics.object_scores restated: fp64 from the table"""
    tab = np.asarray(tab, dtype=np.int64)
    K = tab.shape[0]

    def one(rows):
        nt, npred, tp, s3 = [int(rows[r].sum()) for r in range(4)]
        fn, fp = nt - tp, npred - tp
        nan = float("nan")
        if nt == 0 and npred == 0:
            return dict(truth=0, predicted=0, matched=0, precision=nan, recall=nan, f1=nan, sq=nan, pq=nan)
        f1 = 2.0 * tp / (2.0 * tp + fp + fn)
        sq = s3 / (tp * 2.0 ** 20) if tp else nan
        return dict(truth=nt, predicted=npred, matched=tp, precision=tp / npred if npred else nan, recall=tp / nt if nt else nan,
                    f1=f1, sq=sq, pq=sq * f1 if tp else 0.0)
    return [one(tab[k]) for k in range(K)], one(tab.sum(axis=0))


# ---------------------------------------------------------------------------------------------------------------- inputs
def flipped(m, K, frac=0.08, seed=3):
    """m with a seeded `frac` of the pixels re-drawn to another class"""
    rng = np.random.default_rng(seed)
    hit = rng.random(m.shape) < frac
    out = m.copy()
    out[hit] = (m[hit] + rng.integers(1, K, size=int(hit.sum()))) % K
    return out.astype(np.uint8)


def shifted(m):
    """m moved one pixel down and right, the first row and column repeated"""
    out = m.copy()
    out[1:, 1:] = m[:-1, :-1]
    return out


def with_band(m, x0, x1, byte=6):
    out = m.copy()
    out[:, x0:x1] = byte
    return out


def holed(h=300, w=300, byte=2):
    """(uniform truth, the same with a 60 x 60 square hole of another class): one pair above 65 535 pixels on one vote word"""
    t = sieve_ref.uniform(h, w, byte)
    p = t.copy()
    p[100:160, 120:180] = 1
    return t, p


def cut_serpentine(h=67, w=131):
    """(the corridor, a copy whose corridor is cut in three by two wall pixels): the first piece holds more than half of it"""
    t = sieve_ref.serpentine(h, w)
    p = t.copy()
    p[44, 60] = 0
    p[56, 60] = 0
    return t, p


def fifths():
    """a truth object of 25 x 44 = 1100 pixels under five predicted objects of its class that share it evenly: stripes of 25 x 8 = 200
    pixels (2 / 11 of it each) with one-pixel walls of class 0 between them, without which they would be one object.  No stripe
    holds a majority: match -1, inter 0, whatever candidate the vote leaves"""
    t = np.zeros((27, 46), dtype=np.uint8)
    t[1:26, 1:45] = 1
    p = np.zeros_like(t)
    for s in range(5):
        p[1:26, 1 + 9 * s:9 + 9 * s] = 1
    return t, p


def half_cases():
    """(truth, pred at IoU exactly 1/2, pred with one more shared pixel): |t| = 4, cover = 2, I = 2 -> 3 I = 6 = |t| + cover: no match;
    I = 3, cover = 3: 9 > 7: a match"""
    t = np.zeros((5, 8), dtype=np.uint8)
    t[2, 2:6] = 1
    p2 = np.zeros_like(t)
    p2[2, 2:4] = 1
    p3 = np.zeros_like(t)
    p3[2, 2:5] = 1
    return t, p2, p3


def swallowed():
    """a predicted object that holds ALL of t but is so large that IoU <= 1/2: |t| = 12, |p| = 40, I = 12: 36 > 52 fails"""
    t = np.zeros((8, 12), dtype=np.uint8)
    t[2:5, 2:6] = 1
    p = np.zeros_like(t)
    p[1:6, 1:9] = 1
    return t, p


def band_case():
    """truth with an ignore band (byte 6, columns 20..29) through a 40 x 50 map of class 0 with objects of class 1; pred:
       A rows 2..7,  cols 12..23: 6 x 8 outside the band, 6 x 4 inside; no truth object under it: 2 cover = 96 >= 72: a false positive
       B rows 12..17, cols 18..31: 6 x 2 + 6 x 2 outside, 6 x 10 inside: 2 cover = 48 < 84: dropped
       C rows 22..29, cols 10..25: the truth object rows 22..29, cols 10..19 (80 pixels; the band cuts it) is matched: cover = 80, |p| = 128:
         IoU = 80 / 80 although p reaches 6 columns into the band
       D rows 33..36, cols 24..33: 4 x 4 outside the band, 4 x 6 inside, |p| = 40, cover = 16: it matches the truth object rows 33..36,
         cols 30..33 and so counts as a predicted object although 2 cover < |p|
       and a truth object rows 2..5, cols 40..45 that nothing predicts"""
    t = np.zeros((40, 50), dtype=np.uint8)
    t[22:30, 10:20] = 1
    t[33:37, 30:34] = 1
    t[2:6, 40:46] = 1
    t[:, 20:30] = 6
    p = np.zeros_like(t)
    p[2:8, 12:24] = 1
    p[12:18, 18:32] = 1
    p[22:30, 10:26] = 1
    p[33:37, 24:34] = 1
    return t, p


def beyond_K(h=33, w=65, K=4):
    """a speckled truth of K classes against a prediction that also carries bytes >= K (a bar of 200 and specks of K)"""
    t = sieve_ref.speckled(h, w, K)
    p = flipped(t, K, seed=5)
    p[10:12, 5:60] = 200
    p[20:30:3, 7:60:5] = K
    return t, p


def fixtures():
    """name -> (truth, pred, K, ignore_label, multi): the pairs of the device tests; multi: the fixture must exercise every branch
    (test_object_scores_plan holds it to that)"""
    s = sieve_ref.speckled(45, 131, 6)
    s8 = sieve_ref.speckled(33, 65, 8)
    out = {
        "speckled-flipped": (s, flipped(s, 6), 6, -1, True),
        "speckled-shifted": (s, shifted(s), 6, -1, True),
        "speckled-flipped-band": (with_band(s, 50, 70), flipped(s, 6), 6, 6, True),
        "speckled-33x65-K8": (s8, flipped(s8, 8, seed=4), 8, -1, True),
        "speckled-1x40": (sieve_ref.speckled(1, 40, 3), flipped(sieve_ref.speckled(1, 40, 3), 3, frac=0.2), 3, -1, False),
        "speckled-40x1": (sieve_ref.speckled(40, 1, 3), flipped(sieve_ref.speckled(40, 1, 3), 3, frac=0.2), 3, -1, False),
        "speckled-5x7": (sieve_ref.speckled(5, 7, 2), flipped(sieve_ref.speckled(5, 7, 2), 2, frac=0.2), 2, -1, False),
        "holed-300x300": holed() + (3, -1, False),
        "serpentine-cut": cut_serpentine() + (2, -1, False),
        "fifths": fifths() + (2, -1, False),
        "half-exactly": half_cases()[:2] + (2, -1, False),
        "half-plus-one": (half_cases()[0], half_cases()[2], 2, -1, False),
        "swallowed": swallowed() + (2, -1, False),
        "band": band_case() + (6, 6, True),
        "beyond-K": beyond_K() + (4, -1, True),
    }
    for v in out.values():
        v[0].setflags(write=False)
        v[1].setflags(write=False)
    return out
