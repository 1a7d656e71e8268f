#!/usr/bin/env python3
"""Differential fuzz of the oracle's host half (oracle/host_ref.py) and the product's host functions (drs_amd.patches / sampling /
loops) against the REFERENCE'S OWN FUNCTIONS.  Random inputs, same numpy / random seeds on both sides, exact equality.

Three modes:
    python tests/fuzz/fuzz_vs_reference.py [n=300] [seed=0]              live: the reference imported from make_goldens.REF the way
                                                                         tests/golden/make_goldens.py does (inert placeholders for
                                                                         tensorflow / gdal / skimage; np.int restored)
    python tests/fuzz/fuzz_vs_reference.py n=40 seed=77 record=FILE      live, and the reference's side of every comparison written to
                                                                         FILE (tests/golden/reference_differential.json)
    python tests/fuzz/fuzz_vs_reference.py replay=FILE                   the recorded side instead of the reference: needs nothing
                                                                         outside the repository (tests/test_reference_differential.py)

A recording holds, per comparison, the reference's result as data: small results as values (compared as the live run compares them),
large arrays as a SHA-256 digest of their canonical form (shape + float64 values; what `eq` below calls equal has equal digests).
Nothing of the reference is copied -- it is called, and what it returned is stored."""
import hashlib, json, os, random, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from oracle import host_ref as H
from drs_amd import patches as P
from drs_amd import sampling as SM
from drs_amd import loops as L

ref = None
fails = []


class Recorded(object):
    """the digest of a large reference result (replay mode): equal to an array whose canonical form has the same digest"""
    __slots__ = ("h",)

    def __init__(self, h):
        self.h = h


def digest(x):
    """canonical digest: equal digests <=> `eq` equal (both empty; or same shape and the same values, whatever the numeric dtype).
    None for an array holding a NaN: array_equal never calls it equal to anything."""
    if isinstance(x, str):
        return "s:" + x
    a = np.asarray(x)
    if a.size == 0:
        return "empty"
    f = np.ascontiguousarray(a, dtype=np.float64) + 0.0          # (-0.0 -> 0.0: array_equal does not tell them apart)
    if np.isnan(f).any():
        return None
    return hashlib.sha256(repr(f.shape).encode() + f.tobytes()).hexdigest()


def _enc(x):
    if isinstance(x, np.ndarray):
        return {"nd": x.tolist(), "dtype": x.dtype.str, "shape": list(x.shape)}
    if isinstance(x, np.generic):
        return {"np": x.item(), "dtype": x.dtype.str}
    if isinstance(x, (tuple, list)):
        return {"seq": [_enc(e) for e in x], "tuple": isinstance(x, tuple)}
    if x is None or isinstance(x, (str, bool, int, float)):
        return x
    raise TypeError("cannot record %r" % type(x))


def _dec(x):
    if isinstance(x, dict):
        if "nd" in x:
            return np.array(x["nd"], dtype=np.dtype(x["dtype"])).reshape(x["shape"])
        if "np" in x:
            return np.dtype(x["dtype"]).type(x["np"])
        seq = [_dec(e) for e in x["seq"]]
        return tuple(seq) if x["tuple"] else seq
    return x


class Side(object):
    """the reference's side of the comparisons: called (live / record) or read back (replay), keyed by round and order"""

    def __init__(self, mode, path=None):
        self.mode, self.path, self.records, self.key0, self.k = mode, path, {}, "", 0
        if mode == "replay":
            self.records = json.load(open(path))["records"]

    def round(self, key0):
        self.key0, self.k = key0, 0

    def __call__(self, label, thunk, full=False):
        """`thunk()` computes the reference's result (never called in replay mode).  full=False: a large array or a tuple of them,
        recorded as digests; full=True: a small value, recorded as it is"""
        key = "%s.%d %s" % (self.key0, self.k, label)
        self.k += 1
        if self.mode == "replay":
            if key not in self.records:
                check(label, False, "no recorded result under %r (the comparisons ran in another order)" % key)
                return Recorded(None) if not full else None
            r = self.records[key]
            if "f" in r:
                return _dec(r["f"])
            return tuple(Recorded(h) for h in r["d"]) if isinstance(r["d"], list) else Recorded(r["d"])
        res = thunk()
        if self.mode == "record":
            if full:
                self.records[key] = {"f": _enc(res)}
            else:
                self.records[key] = {"d": [digest(e) for e in res] if isinstance(res, tuple) else digest(res)}
        return res

    def save(self, n, seed):
        with open(self.path, "w") as f:
            json.dump({"n": n, "seed": seed, "note": "the reference's results in tests/fuzz/fuzz_vs_reference.py n=%d seed=%d: values, or "
                       "SHA-256 digests of the canonical form (shape + float64 values) for large arrays" % (n, seed),
                       "records": self.records}, f, indent=0, sort_keys=True)
            f.write("\n")


R = Side("live")


def check(name, ok, detail=""):
    if not ok:
        fails.append((name, detail))
        print("FAIL", name, detail, flush=True)


def eq(a, b):
    if isinstance(a, Recorded):
        return a.h is not None and a.h == digest(b)
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0 and b.size == 0:           # (an empty batch: the reference returns [] where the build returns shape (0, 2))
        return True
    return a.shape == b.shape and np.array_equal(a, b)


def _seeded(seed, f, both=False):
    np.random.seed(seed)
    if both:
        random.seed(seed)
    return f()


def _mutated(f, arg):
    f(arg)
    return arg


def one(rng, i):
    R.round("%d" % i)
    # ---- crop + augmentation
    C = int(rng.choice([3, 4, 5]))
    h, w = int(rng.integers(30, 120)), int(rng.integers(30, 120))
    S = int(rng.integers(5, min(h, w, 35) + 1))
    B = int(rng.integers(1, 7))
    tiles = [rng.uniform(size=(h, w, C)) for _ in range(2)]
    labs = [rng.integers(0, 6, size=(h, w)) for _ in range(2)]
    inst = np.stack([rng.integers(0, 2, size=B), rng.integers(0, h - 1, size=B), rng.integers(0, w - 1, size=B), rng.integers(0, 360, size=B)], 1)
    for train in (False, True):
        seed = int(rng.integers(0, 2 ** 31))
        a = R("dynamically_create_patches", lambda: tuple(_seeded(seed, lambda: ref.dynamically_create_patches(tiles, labs, inst, S, is_train=train))))
        np.random.seed(seed)
        b = H.dynamically_create_patches(tiles, labs, inst, S, is_train=train)
        check("dynamically_create_patches", all(eq(x, y) for x, y in zip(a, b)), "train=%s S=%d %dx%d" % (train, S, h, w))
    mean, std = rng.uniform(0.2, 0.6, size=C), rng.uniform(0.1, 0.4, size=C)
    x1 = rng.uniform(size=(B, S, S, C)); x2 = x1.copy()
    a = R("normalize_images", lambda: _mutated(lambda x: ref.normalize_images(x, mean, std), x1.copy()))
    H.normalize_images(x2, mean, std)
    check("normalize_images", eq(a, x2))
    # ---- windows
    S2 = int(rng.integers(4, 34)); st = int(rng.integers(1, S2 + 1))
    h2, w2 = int(rng.integers(S2, S2 + 80)), int(rng.integers(S2, S2 + 80))
    bs = int(rng.integers(1, 40))
    tile = rng.uniform(size=(h2, w2, 2)); lab = rng.integers(0, 6, size=(h2, w2))
    nh, nw = H.window_counts(h2, w2, S2, st)
    idx = int(rng.integers(0, max(1, -(-nh * nw // bs))))
    a = R("create_patches_per_map", lambda: (lambda r: (r[0], r[1], np.asarray(r[2])))(ref.create_patches_per_map(tile, lab, S2, st, idx, bs)))
    b = H.create_patches_per_map(tile, lab, S2, st, idx, bs)
    check("create_patches_per_map", eq(a[0], b[0]) and eq(a[1], b[1]) and eq(a[2], np.asarray(b[2])), "%dx%d S%d st%d idx%d bs%d" % (h2, w2, S2, st, idx, bs))
    # (a[2] as int64: the same canonical form, so the same digest)
    check("window_positions", eq(a[2] if isinstance(a[2], Recorded) else np.asarray(a[2]).astype(np.int64), P.window_positions(h2, w2, S2, st, idx, bs)),
          "%dx%d S%d st%d idx%d bs%d" % (h2, w2, S2, st, idx, bs))
    # ---- accuracy / confusion
    K = 6
    t = rng.integers(0, K, size=(B, S, S)); p = rng.integers(0, K, size=(B, S, S)); m = rng.integers(0, 2, size=(B, S, S)).astype(bool)
    c2 = np.zeros((K, K), dtype=np.uint32)

    def ref_acc():
        c1 = np.zeros((K, K), dtype=np.uint32)
        r = ref.calc_accuracy_by_crop(t, p, c1, m)
        return (r[0], r[1], r[2], c1)
    a = R("calc_accuracy_by_crop", ref_acc, full=True)
    b = H.calc_accuracy_by_crop(t, p, c2, m, K)
    check("calc_accuracy_by_crop", eq(a[0], b[0]) and np.allclose(a[1], b[1], rtol=0, atol=0) and eq(a[2], b[2]) and eq(a[3], c2))
    # ---- batch walk
    n = int(rng.integers(3, 60)); bsz = int(rng.integers(1, n + 1)); it = int(rng.integers(0, n)); sd = int(rng.integers(0, 10 ** 6))
    sh = rng.permutation(n)
    a = R("select_batch", lambda: tuple(_seeded(sd, lambda: ref.select_batch(sh.copy(), bsz, it, n), both=True)))
    random.seed(sd); np.random.seed(sd)
    b = H.select_batch(sh.copy(), bsz, it, n)
    random.seed(sd); np.random.seed(sd)
    c = P.select_batch(sh.copy(), bsz, it, n)
    check("select_batch", all(eq(x, y) for x, y in zip(a, b)) and all(eq(x, y) for x, y in zip(a, c)), "n=%d bs=%d it=%d" % (n, bsz, it))
    # ---- size distributions and the best-size rule
    v0 = int(rng.integers(20, 40)); vals = sorted(set(int(v) for v in rng.integers(v0, v0 + 80, size=int(rng.integers(2, 6)))))
    if len(vals) >= 2:
        def attempt(f):
            try:
                return f(vals)
            except ZeroDivisionError:        # the reference divides by interval - len(values): consecutive values leave nothing to share
                return "ZeroDivisionError"
        ra = R("define_multinomial_probs", lambda: attempt(ref.define_multinomial_probs), full=True)
        rb, rc = attempt(H.define_multinomial_probs), attempt(P.define_multinomial_probs)
        check("define_multinomial_probs", (isinstance(ra, str) and ra == rb == rc) or (not isinstance(ra, str) and eq(ra, rb) and eq(ra, rc)), str(vals))
        for dist in ("multi_fixed", "uniform", "multinomial"):
            ln = len(vals) if dist == "multi_fixed" else vals[-1] - vals[0] + 1
            sums = rng.uniform(0, 5, size=ln).astype(np.float32); cnt = rng.integers(0, 4, size=ln).astype(np.int32)
            for kind in ("acc", "loss"):
                c2, c3 = cnt.copy(), cnt.copy()

                def ref_best():
                    c1 = cnt.copy()
                    return (ref.select_best_patch_size(dist, vals, sums.copy(), c1, kind), c1)
                a, c1 = R("select_best_patch_size", ref_best, full=True)
                b = H.select_best_patch_size(dist, vals, sums.copy(), c2, kind)
                c = L.select_best_patch_size(dist, vals, sums.copy(), c3, kind)
                check("select_best_patch_size", a == b == c and eq(c1, c2) and eq(c1, c3), "%s %s %s" % (dist, kind, vals))
    # ---- class distributions, super-batches, mean / std
    if i % 5 == 0:
        labs2 = [rng.integers(0, 6, size=(int(rng.integers(40, 90)), int(rng.integers(40, 90)))) for _ in range(2)]
        cs, sc = int(rng.integers(8, 26)), int(rng.integers(3, 20))
        a_live = []

        def ref_dist():
            a_live[:] = ref.create_distributions_over_classes(labs2, cs, sc)
            return tuple(np.asarray(x).reshape(-1, 3) if len(x) else np.zeros((0, 3)) for x in a_live)
        a = R("create_distributions_over_classes", ref_dist)
        b = SM.create_distributions_over_classes(labs2, cs, sc)
        check("create_distributions_over_classes", len(a) == len(b) and all(eq(x, np.asarray(y).reshape(-1, 3) if len(y) else np.zeros((0, 3))) for x, y in zip(a, b)), "crop %d stride %d" % (cs, sc))
        # (what follows is run where the product's distributions are non-empty: equal to the reference's, checked just above)
        if all(len(x) > 0 for x in b):
            sd = int(rng.integers(0, 10 ** 6))

            def ref_super():
                np.random.seed(sd); random.seed(sd)
                rot_a = ref.create_rotation_distribution(a_live)
                return np.asarray(ref.select_super_batch_instances(a_live, rot_a, batch_size=12, super_batch=5))
            ia = R("select_super_batch_instances", ref_super)
            np.random.seed(sd); random.seed(sd)
            rot_b = SM.create_rotation_distribution(b)
            ib = SM.select_super_batch_instances(b, rot_b, batch_size=12, super_batch=5)
            check("select_super_batch_instances", eq(ia, np.asarray(ib)))
            data = [rng.uniform(size=(l.shape[0], l.shape[1], 4)) for l in labs2]
            ma = R("dynamically_calculate_mean_and_std", lambda: tuple(ref.dynamically_calculate_mean_and_std(data, a_live, cs)))
            mb = SM.dynamically_calculate_mean_and_std(data, b, cs)
            check("dynamically_calculate_mean_and_std", all(eq(x, y) for x, y in zip(ma, mb)))


_flav = {}


def flavours(rng, i):
    """coffee_dilated_random.py / contest_dilated_random.py: class distributions (with their quirks), mean / std, the flip-by-index
    sampler (float16 cast; void mask), window enumeration -- the reference's functions against drs_amd.loops_indexed /
    oracle.host_ref / drs_amd.patches"""
    import importlib
    from drs_amd import loops_indexed as LI
    R.round("f%d" % i)
    if not _flav and R.mode != "replay":
        from make_goldens import _NpPy2
        _flav["cf"] = importlib.import_module("coffee_dilated_random")
        _flav["cf"].np = _NpPy2()
        _flav["ct"] = importlib.import_module("contest_dilated_random")
    cf, ct = _flav.get("cf"), _flav.get("ct")
    # ---- coffee: square tiles, binary masks
    n, hw = int(rng.integers(1, 4)), int(rng.integers(24, 60))
    data = rng.uniform(0, 1, size=(n, hw, hw, 3)).astype(np.float32)
    mask = np.zeros((n, hw, hw, 1), dtype=np.float32)
    for k in range(n):
        for _ in range(int(rng.integers(1, 4))):
            a, b, c, d = sorted(rng.integers(0, hw, size=2)), sorted(rng.integers(0, hw, size=2)), 0, 0
            mask[k, a[0]:a[1] + 1, b[0]:b[1] + 1] = 1
    cs, st = int(rng.integers(5, 12)), int(rng.integers(2, 8))
    da_live = []

    def ref_cdist():
        da_live[:] = cf.create_distributions_over_classes([mask[k] for k in range(n)], cs, st)
        return np.array([(k, i, j) for (k, (i, j)) in da_live], dtype=np.int64).reshape(-1, 3)
    flat = R("coffee create_distributions_over_classes", ref_cdist)
    db = LI.create_distributions_over_classes([mask[k] for k in range(n)], cs, st, 2)
    flat_b = np.asarray(db, dtype=np.int64).reshape(-1, 3)
    check("coffee create_distributions_over_classes", eq(flat, flat_b), "crop %d stride %d" % (cs, st))
    ma = R("coffee create_mean_and_std", lambda: tuple(cf.create_mean_and_std(data, mask, cs, st)), full=True)
    mb = LI.create_mean_and_std(data, cs, st)
    check("coffee create_mean_and_std", np.allclose(ma[0], mb[0], rtol=2e-6, atol=0) and np.allclose(ma[1], mb[1], rtol=2e-6, atol=0))
    # (the product's distribution list, equal to the reference's (checked above), drives the rest)
    if len(flat_b):
        nd = len(flat_b)
        shuffle = rng.integers(0, 3 * nd, size=int(rng.integers(1, 12)))
        S = int(rng.integers(cs, min(hw, cs + 8) + 1))
        pa_live = []

        def ref_cpatch():
            pa, ca = cf.dynamically_create_patches(data, mask, S, da_live, shuffle)
            pa_live[:] = [pa]
            return (str(pa.dtype), pa, ca[..., 0])
        pa = R("coffee dynamically_create_patches", ref_cpatch)
        pb, cb, _ = H.indexed_create_patches(data, mask[..., 0], S, [(int(k), int(i), int(j)) for k, i, j in flat_b], shuffle, float16=True)
        check("coffee dynamically_create_patches", eq(pa[0], str(pb.dtype)) and eq(pa[1], pb) and eq(pa[2], cb), "S %d" % S)
        qa = R("coffee normalize_images", lambda: _mutated(lambda q: cf.normalize_images(q, ma[0], ma[1]), pa_live[0].copy()))
        check("coffee normalize_images (float16, in place)", eq(qa, H.normalize_images_f16(pb, ma[0], ma[1])))
    S2 = int(rng.integers(5, 16)); st2 = int(rng.integers(2, S2 + 1)); bs = int(rng.integers(1, 30))
    nw = H.window_counts(hw, hw, S2, st2)
    idx = int(rng.integers(0, max(1, -(-nw[0] * nw[1] // bs))))
    pos = R("coffee window positions", lambda: np.asarray(cf.create_patches_per_map(data[0], mask[0], S2, st2, idx, bs)[2]).astype(np.int64))
    check("coffee window positions", eq(pos, P.window_positions(hw, hw, S2, st2, idx, bs, "coffee")), "%d S%d st%d idx%d bs%d" % (hw, S2, st2, idx, bs))
    # ---- contest: one non-square tile, 7 classes + void (7)
    h, w = int(rng.integers(30, 70)), int(rng.integers(30, 70))
    img = rng.uniform(0, 1, size=(h, w, 3)).astype(np.float32)
    lab = rng.integers(0, 7, size=(h, w)).astype(np.int64)
    for _ in range(int(rng.integers(0, 4))):            # uniform regions and void regions: where the quirks live
        a, b = sorted(rng.integers(0, h, size=2)), sorted(rng.integers(0, w, size=2))
        lab[a[0]:a[1] + 1, b[0]:b[1] + 1] = int(rng.integers(0, 8))
    da_live = []

    def ref_tdist():
        da_live[:] = ct.create_distributions_over_classes(lab, cs, st)
        return np.array(da_live, dtype=np.int64).reshape(-1, 2)
    fa = R("contest create_distributions_over_classes", ref_tdist)
    db = LI.create_distributions_over_classes_contest(lab, cs, st)
    fa_b = np.asarray(db, dtype=np.int64).reshape(-1, 3)[:, 1:]
    check("contest create_distributions_over_classes", eq(fa, fa_b), "crop %d stride %d" % (cs, st))
    if len(fa_b):
        ma = R("contest create_mean_and_std", lambda: tuple(ct.create_mean_and_std(img, da_live, cs)), full=True)
        mb = LI.create_mean_and_std_contest(img, db, cs)
        check("contest create_mean_and_std", np.allclose(ma[0], mb[0], rtol=2e-6, atol=0) and np.allclose(ma[1], mb[1], rtol=2e-6, atol=0))
        nd = len(fa_b)
        shuffle = rng.integers(0, 3 * nd, size=int(rng.integers(1, 12)))
        S = int(rng.integers(cs, min(h, w, cs + 8) + 1))
        pa = R("contest dynamically_create_patches", lambda: tuple(ct.dynamically_create_patches(img, lab, S, da_live, shuffle)))
        pb, cb, qb = H.indexed_create_patches(img[None], lab[None], S, [(0, int(i), int(j)) for i, j in fa_b], shuffle, void_label=7)
        check("contest dynamically_create_patches", eq(pa[0], pb) and eq(pa[1], cb) and eq(pa[2], qb), "S %d" % S)
    nh, nw2 = H.window_counts(h, w, S2, st2)
    idx = int(rng.integers(0, max(1, -(-nh * nw2 // bs))))

    def ref_tpos():
        try:
            return np.asarray(ct.create_patches_per_map(img, lab, S2, st2, idx, bs)[3]).astype(np.int64)
        except Exception:                               # (contest:275's start index can run off a non-square tile)
            return None
    ran = R("contest window positions ran", lambda: ref_tpos() is not None, full=True)
    if ran:
        res = R("contest window positions", ref_tpos)
        check("contest window positions", eq(res, P.window_positions(h, w, S2, st2, idx, bs, "contest")), "%dx%d S%d st%d idx%d bs%d" % (h, w, S2, st2, idx, bs))


def main(n=300, seed=0, record=None, replay=None):
    global ref, R
    if replay:
        R = Side("replay", replay)
        rec = json.load(open(replay))
        n, seed = rec["n"], rec["seed"]
    else:
        from make_goldens import REF, import_reference
        if not os.path.isdir(REF):
            print("the reference is not here: nothing to compare against (replay=tests/golden/reference_differential.json compares "
                  "against the recorded results)")
            sys.exit(0)
        ref = import_reference()
        R = Side("record" if record else "live", record)
    rng = np.random.default_rng(seed)
    for i in range(n):
        one(rng, i)
        if i % 2 == 0:
            flavours(rng, i)
    if record:
        R.save(n, seed)
    names = sorted(set(f[0] for f in fails))
    print("%d rounds against the reference's %s: %d mismatches%s" % (n, "recorded results" if replay else "own functions", len(fails),
                                                                      (" in " + ", ".join(names)) if names else ""))
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(int(kw.get("n", 300)), int(kw.get("seed", 0)), kw.get("record"), kw.get("replay"))
