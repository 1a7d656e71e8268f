"""Host side of the exact test of the pooled batch-norm kernels (tests/test_gpu_pool_exact.py): the numpy reference
(tests/pool_exact_ref.py) against the oracle's pool and activation, the exactness of its input grid in fp32, the density of ties the
grid produces, and the restated strip geometry against the shape table of the GPU test.  No GPU."""
import re
import os

import numpy as np
import pytest

from oracle import tf_ops as T

import pool_exact_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------- reference against the oracle
@pytest.mark.parametrize("B,S,C", [(2, 1, 8), (2, 2, 8), (3, 5, 12), (2, 19, 8)])
@pytest.mark.parametrize("kind,alpha", [("relu", 0.0), ("lrelu", 0.1)])
def test_reference_equals_the_oracle(B, S, C, kind, alpha):
    """the oracle's activation knows two slopes, 0 (relu) and 0.1 (lrelu): those are compared as a whole chain, and the grid's 0.25
    through the pool alone (below)"""
    z, mr, g = R.exact_inputs(B, S, C, seed=S)
    ref = R.reference(z, mr, alpha, g)
    xhat = (z.astype(np.float64) - mr[:, 0].astype(np.float64)) * mr[:, 1].astype(np.float64)
    a = T.act_fwd(xhat, kind)
    out, idx = T.max_pool_3x3(a)
    assert np.array_equal(ref["a"], a) and np.array_equal(ref["out"], out)
    assert np.array_equal(ref["idx"], idx)
    gpool = T.max_pool_3x3_bwd(idx, g.astype(np.float64))
    assert np.array_equal(ref["gpool"], gpool)
    gx = T.act_bwd(xhat, kind, gpool)
    assert np.array_equal(ref["gxhat"], gx)
    assert np.array_equal(ref["sum_g"], gx.sum(axis=(0, 1, 2))) and np.array_equal(ref["sum_gx"], (gx * xhat).sum(axis=(0, 1, 2)))


@pytest.mark.parametrize("alpha", R.ALPHAS)
def test_reference_pool_equals_the_oracle_pool_on_the_grid(alpha):
    z, mr, g = R.exact_inputs(3, 7, 8, seed=11)
    ref = R.reference(z, mr, alpha, g)
    out, idx = T.max_pool_3x3(ref["a"])
    assert np.array_equal(ref["out"], out) and np.array_equal(ref["idx"], idx)
    assert np.array_equal(ref["gpool"], T.max_pool_3x3_bwd(idx, g.astype(np.float64)))
    # the activation's backward with the oracle's decision, the slope applied here
    assert np.array_equal(ref["gxhat"], np.where(T.act_bwd(ref["xhat"], "relu", np.ones_like(ref["xhat"])) > 0, ref["gpool"], ref["gpool"] * alpha))


def test_reference_on_a_hand_made_patch():
    """3 x 3, one channel, mean 0, rstd 1: every code by hand"""
    z = np.array([[1, 1, 0], [0, 1, 0], [0, 0, -1]], dtype=np.float32).reshape(1, 3, 3, 1)
    mr = np.array([[0.0, 1.0]], dtype=np.float32)
    g = np.arange(1, 10, dtype=np.float32).reshape(1, 3, 3, 1)
    ref = R.reference(z, mr, 0.0, g, want_count=True)
    assert ref["out"][0, :, :, 0].tolist() == [[1, 1, 1], [1, 1, 1], [1, 1, 1]]
    # window scan order: row above first, left to right; padding never wins
    assert ref["idx"][0, :, :, 0].tolist() == [[4, 3, 3], [1, 0, 0], [2, 1, 0]]
    assert ref["count"][0, :, :, 0].tolist() == [[3, 3, 2], [3, 3, 2], [1, 1, 1]]
    # input (0,0) <- outputs (0,0) (0,1) (1,0) (1,1); (0,1) <- (0,2) (1,2); (1,1) <- the bottom row
    assert ref["gpool"][0, :, :, 0].tolist() == [[1 + 2 + 4 + 5, 3 + 6, 0], [0, 7 + 8 + 9, 0], [0, 0, 0]]
    assert np.array_equal(ref["gxhat"], ref["gpool"])          # relu: every input that received something is positive
    assert ref["sum_g"][0] == 45 and ref["sum_gx"][0] == 45
    # leaky: the same routing; a non-positive input would pass alpha times what it receives
    z2 = z.copy()
    z2[0, 1, 1, 0] = -2.0                                     # a = -0.5: the bottom row's windows now tie at zero
    ref = R.reference(z2, mr, 0.25, g)
    assert ref["idx"][0, :, :, 0].tolist() == [[4, 3, 3], [1, 0, 0], [1, 0, 1]]
    assert ref["gpool"][0, :, :, 0].tolist() == [[1 + 2 + 4 + 5, 3 + 6, 0], [7 + 8, 0, 9], [0, 0, 0]]
    assert ref["gxhat"][0, :, :, 0].tolist() == [[12, 9, 0], [15 * 0.25, 0, 9 * 0.25], [0, 0, 0]]
    assert ref["sum_g"][0] == 27 and ref["sum_gx"][0] == 21


def test_sign_of_a_zero_maximum():
    """alpha = 0: negative inputs become -0.0, a zero input +0.0.  Windows of -0.0 only must give -0.0, windows of +0.0 only +0.0, and
    only windows that hold both are free"""
    z = np.full((1, 7, 7, 1), -1.0, dtype=np.float32)
    z[0, :, 5:, 0] = 0.0
    ref = R.reference(z, np.array([[0.0, 1.0]], dtype=np.float32), 0.0)
    assert np.all(ref["out"] == 0)
    for y in range(7):
        assert ref["zero_free"][0, y, :, 0].tolist() == [False, False, False, False, True, True, False]
        assert np.signbit(ref["out"][0, y, :, 0]).tolist() == [True, True, True, True, False, False, False]
    assert not R.reference(z, np.array([[0.0, 1.0]], dtype=np.float32), 0.25)["zero_free"].any()


# ------------------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("B,S,C", [(4, 5, 16), (3, 19, 8), (2, 33, 8)])
def test_the_chain_in_fp32_is_the_chain_in_fp64(B, S, C, alpha):
    z, mr, g = R.exact_inputs(B, S, C, seed=B + S)
    r64, r32 = R.reference(z, mr, alpha, g), R.reference(z, mr, alpha, g, dtype=np.float32)
    for k in ("xhat", "a", "out", "gpool", "gxhat"):
        assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64
        assert np.array_equal(_bits(r32[k]), _bits(r64[k])), k           # the sign of every zero included
    assert np.array_equal(r32["idx"], r64["idx"]) and np.array_equal(r32["zero_free"], r64["zero_free"])
    # the terms of the two sums, and the sums of a whole patch (more pixels than any workgroup of the table) in fp32 in three orders
    t32, t64 = r32["gxhat"] * r32["xhat"], r64["gxhat"] * r64["xhat"]
    assert np.array_equal(_bits(t32), _bits(t64))
    assert np.abs(t64).max() <= R.MAX_ABS_TERM and np.array_equal(t64 / R.TERM_UNIT, np.round(t64 / R.TERM_UNIT))
    assert S * S <= R.MAX_EXACT_PIXELS
    for v32, v64 in ((r32["gxhat"], r64["gxhat"]), (t32, t64)):
        want = v64.sum(axis=(1, 2))
        flat = v32.reshape(B, S * S, C)
        seq = np.zeros((B, C), dtype=np.float32)
        for p in range(S * S):
            seq += flat[:, p]
        assert seq.dtype == np.float32
        for got in (seq, flat.sum(axis=1, dtype=np.float32), flat[:, ::-1].sum(axis=1, dtype=np.float32)):
            assert np.array_equal(got.astype(np.float64), want)
    # an FMA of exact operands: the products are exact, so fusing the multiply into the add changes nothing
    fma = np.zeros((B, C), dtype=np.float64)
    for p in range(S * S):
        fma = (fma + r64["gxhat"].reshape(B, S * S, C)[:, p] * r64["xhat"].reshape(B, S * S, C)[:, p]).astype(np.float32).astype(np.float64)
    assert np.array_equal(fma, t64.sum(axis=(1, 2)))


def test_every_workgroup_of_the_table_sums_exactly():
    for name, shape, sw, alpha, want in R.CASES:
        geo = R.case_geometry(shape, sw)
        pixels = geo["pixels"] if geo else 256                  # the gathering form: at most 256 pixels per workgroup
        assert pixels < R.MAX_EXACT_PIXELS // 4, name


# ------------------------------------------------------------------------------------------------- tie density
@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("S", [5, 19, 33])
def test_the_grid_is_dense_in_ties(S, alpha):
    z, mr, g = R.exact_inputs(4, S, 64, seed=S)
    ref = R.reference(z, mr, alpha, want_count=True)
    share, share_pos, tie = R.tie_stats(ref)
    assert share >= 0.20 and share_pos >= 0.15, (share, share_pos)
    # zero maxima over zeros of both signs, whose sign is free, stay rare: the sign of a zero is checked nearly everywhere
    assert ref["zero_free"].mean() < 0.03 and (alpha == 0.0) == bool(ref["zero_free"].any())
    assert sorted(np.unique(ref["idx"]).tolist()) == list(range(9))
    pos = tie & (ref["out"] > 0)
    for edge in (pos[:, 0], pos[:, -1], pos[:, :, 0], pos[:, :, -1]):
        assert edge.any()
    # ties whose first maximum is in each of the three window rows and columns: every arm of the kernels' selects decides some tie
    codes = ref["idx"][pos]
    assert sorted(np.unique(codes // 3).tolist()) == [0, 1, 2] and sorted(np.unique(codes % 3).tolist()) == [0, 1, 2]


@pytest.mark.parametrize("S", [1, 2])
def test_tiny_sides_have_ties_too(S):
    z, mr, g = R.exact_inputs(3, S, 64, seed=S)
    ref = R.reference(z, mr, 0.25, want_count=True)
    if S == 1:
        assert np.all(ref["idx"] == 4) and np.all(ref["count"] == 1)
    else:
        assert R.tie_stats(ref)[0] > 0.1
        # padding never wins: output (0,0) sees taps 4 5 7 8, (0,1) 3 4 6 7, (1,0) 1 2 4 5, (1,1) 0 1 3 4
        for (y, x), ok in {(0, 0): {4, 5, 7, 8}, (0, 1): {3, 4, 6, 7}, (1, 0): {1, 2, 4, 5}, (1, 1): {0, 1, 3, 4}}.items():
            assert set(np.unique(ref["idx"][:, y, x]).tolist()) == ok


# ------------------------------------------------------------------------------------------------- geometry
def test_the_restated_rule_reads_like_the_source():
    """the constants of slide_cfg that the restatement copies are still in pointwise.hip"""
    src = open(os.path.join(ROOT, "dynamic-rs-segmentation_amd", "csrc", "pointwise.hip")).read()
    m = re.search(r"static int g_slide_blocks = (\d+), g_slide_minrows = (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (R.SLIDE_BLOCKS, R.SLIDE_MINROWS)
    body = src[src.index("static SlideCfg slide_cfg("):src.index("// zero the halo of a view")]
    for piece in ("c.TX = 256 / CQ;", "c.ncol = (S + c.TX - 1) / c.TX;",
                  "c.nstrips < g_slide_blocks && S / (c.nstrips * 2) >= g_slide_minrows) c.nstrips *= 2;",
                  "c.nstrips < 768 && S / (c.nstrips * 2) >= 2) c.nstrips *= 2;", "c.rps = (S + c.nstrips - 1) / c.nstrips;"):
        assert piece in body, piece
    assert "static bool slide_ok(int C) { return C / 4 <= 128; }" in src


def test_geometry_by_hand():
    g = R.slide_geometry(128, 64, 64)                     # the timed step: 512 -> 1024 -> 2048 -> 4096 workgroups, then 64 / 16 < 8
    assert (g["TX"], g["ncol"], g["nstrips"], g["rps"], g["empty"]) == (16, 4, 8, 8, 0)
    g = R.slide_geometry(128, 64, 256)                    # 2048 -> 4096 -> 8192 workgroups: 16-row strips
    assert (g["TX"], g["ncol"], g["nstrips"], g["rps"], g["empty"]) == (4, 16, 4, 16, 0)
    g = R.slide_geometry(12, 33, 128)
    assert (g["TX"], g["ncol"], g["nstrips"], g["rps"]) == (8, 5, 16, 3) and g["rows"] == [3] * 11 + [0] * 5
    assert R.slide_geometry(1, 5, 576) is None and R.slide_geometry(1, 5, 512)["TX"] == 2


def test_the_shape_table_reaches_every_class():
    geos = {}
    for name, shape, sw, alpha, want in R.CASES:
        geo = R.case_geometry(shape, sw)
        geos[name] = geo
        print("%-32s %-16s @ %-12s alpha %-4s %s" % (name, shape, sw, alpha, R.describe(geo)))
        if want is None:
            assert geo is None, name
            continue
        live = [n for n in geo["rows"] if n]
        assert (geo["nstrips"], geo["rps"], live[-1], geo["empty"]) == want, (name, R.describe(geo))
        assert sum(geo["rows"]) == shape[1] and geo["rows"] == live + [0] * geo["empty"]
        assert geo["workgroups"] == shape[0] * geo["ncol"] * geo["nstrips"]
        assert alpha in R.ALPHAS
    # one long strip: every remainder of the ring of three, at least five whole turns
    assert sorted(geos[n]["rps"] % 3 for n in ("one_strip_rows_0_mod_3", "one_strip_rows_1_mod_3", "one_strip_rows_2_mod_3")) == [0, 1, 2]
    assert all(geos[n]["rps"] >= 15 for n in geos if n.startswith("one_strip"))
    # strips of 9 or more rows (three turns), which no other op-level test reaches
    assert geos["two_uneven_strips"]["rows"] == [9, 8]
    assert geos["four_strips"]["rows"] == [5, 5, 5, 2]
    assert geos["one_row_strips"]["rows"] == [1] * 16
    g = geos["two_columns_224_threads"]
    assert g["TX"] == 2 and g["threads"] == 224 and g["threads"] % 64
    assert geos["empty_strips"]["empty"] == 5 and geos["empty_strip_and_one_row_strip"]["rows"][-2:] == [1, 0]
    g = geos["more_columns_than_the_patch"]
    assert g["TX"] > 5 and g["ncol"] == 1
    assert geos["columns_tile_the_side_two"]["tiles"] and geos["columns_tile_the_side_four"]["tiles"]
    assert geos["columns_tile_the_side_two"]["TX"] == 2 and geos["columns_tile_the_side_four"]["TX"] == 4
    overhang = [n for n, g in geos.items() if g and not g["tiles"]]
    assert len(overhang) >= 8
    # column blocks in the middle of a row (neither the first nor the last) exist: both exchange cells come from neighbours
    assert any(g and g["ncol"] >= 3 for g in geos.values())
    assert {s[1] for n, s, sw, a, w in R.CASES} >= {1, 2}
    # both slopes in every family of classes
    for fam in ("one_strip", "columns_tile", "side_1", "side_2"):
        assert {a for n, s, sw, a, w in R.CASES if n.startswith(fam)} == set(R.ALPHAS), fam
    # the invariance shape really has three geometries
    rows = [R.case_geometry(R.INVARIANCE_SHAPE, sw)["rows"] for sw in R.INVARIANCE_SETTINGS]
    assert rows == [[17], [9, 8], [5, 5, 5, 2]]


def test_slide_partials_add_up():
    z, mr, g = R.exact_inputs(3, 7, 16, seed=2)
    ref = R.reference(z, mr, 0.25, g)
    geo = R.slide_geometry(3, 7, 16, blocks=5120, minrows=1)
    assert geo["nstrips"] == 4 and geo["rows"] == [2, 2, 2, 1] and geo["TX"] == 64
    geo = dict(geo, TX=3, ncol=3)                   # (column blocks of three: the arithmetic of the slab rows, not a real launch)
    p = R.slide_partials(ref["gxhat"], ref["xhat"], geo)
    assert p.shape == (3 * 4 * 3, 16, 2)
    assert np.array_equal(p[:, :, 0].sum(axis=0), ref["sum_g"]) and np.array_equal(p[:, :, 1].sum(axis=0), ref["sum_gx"])
    assert np.array_equal(p[(1 * 4 + 3) * 3 + 2, :, 0], ref["gxhat"][1, 6:7, 6:7].sum(axis=(0, 1)))
