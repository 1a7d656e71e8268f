"""CPU: the pieces of dihedral test-time augmentation (loops.predict_tile_dense's tta) that need no GPU -- the numpy statement of the 8
symmetries of the square (patches.dihedral_index / dihedral_apply), the group names, the symmetric-margin tile plan and the isprs
command line's --dense-tta flag."""
import itertools

import numpy as np
import pytest


def _perm(idx, T):
    """a [T][T] pair of index arrays as one flat permutation of T * T"""
    return (idx[0] * T + idx[1]).reshape(-1)


def test_dihedral_index_is_eight_distinct_permutations_with_identity_first():
    from drs_amd import patches as P
    for T in (1, 2, 3, 5, 8):
        fwd = [_perm(P.dihedral_index(g, T)[0], T) for g in range(8)]
        for p in fwd:
            assert sorted(p.tolist()) == list(range(T * T))
        np.testing.assert_array_equal(fwd[0], np.arange(T * T))
        if T >= 2:
            assert len({tuple(p) for p in fwd}) == 8, T


def test_dihedral_index_matches_the_definition():
    from drs_amd import patches as P
    T = 7
    X = np.arange(T * T).reshape(T, T)
    for g in range(8):
        fx, fy, t = g & 1, (g >> 1) & 1, (g >> 2) & 1
        (I, J), (Ii, Ji) = P.dihedral_index(g, T)
        for i in range(T):
            for j in range(T):
                i2, j2 = (T - 1 - i if fy else i), (T - 1 - j if fx else j)
                assert (I[i, j], J[i, j]) == ((j2, i2) if t else (i2, j2))
                a2, b2 = (j, i) if t else (i, j)            # inverse: transpose first, then flip
                assert (Ii[i, j], Ji[i, j]) == ((T - 1 - a2 if fy else a2), (T - 1 - b2 if fx else b2))
        Z = X.swapaxes(0, 1) if t else X
        np.testing.assert_array_equal(X[I, J], Z[::-1 if fy else 1, ::-1 if fx else 1])
        np.testing.assert_array_equal(P.dihedral_apply(X, g), X[I, J])
    # the crop's flip codes: flip 1 (flipud) = g 2, flip 2 (fliplr) = g 1
    np.testing.assert_array_equal(P.dihedral_apply(X, 2), np.flipud(X))
    np.testing.assert_array_equal(P.dihedral_apply(X, 1), np.fliplr(X))
    np.testing.assert_array_equal(P.dihedral_apply(X, 3), np.rot90(X, 2))


def test_inverse_undoes_every_code_and_the_quarter_turns_are_not_self_inverse():
    from drs_amd import patches as P
    for T in (1, 2, 4, 5, 9, 16):
        ident = np.arange(T * T)
        for g in range(8):
            (I, J), (Ii, Ji) = P.dihedral_index(g, T)
            f, inv = _perm((I, J), T), _perm((Ii, Ji), T)
            np.testing.assert_array_equal(f[inv], ident)      # sigma_g^-1 then sigma_g
            np.testing.assert_array_equal(inv[f], ident)
            if T >= 2:
                assert np.array_equal(f, inv) == (g not in (5, 6)), (T, g)
    # on non-square arrays too: g^-1 . g = id
    x = np.random.default_rng(0).normal(size=(5, 9, 3))
    for g in range(8):
        y = P.dihedral_apply(x, g)
        assert y.shape == ((9, 5, 3) if g & 4 else x.shape)
        np.testing.assert_array_equal(P.dihedral_apply(y, g, inverse=True), x)


def test_the_eight_codes_form_a_group():
    from drs_amd import patches as P
    T = 6
    fwd = [_perm(P.dihedral_index(g, T)[0], T) for g in range(8)]
    table = {tuple(p): g for g, p in enumerate(fwd)}
    for a, b in itertools.product(range(8), repeat=2):
        assert tuple(fwd[a][fwd[b]]) in table, (a, b)          # closed under composition
    for a in range(8):
        inv = np.argsort(fwd[a])
        assert tuple(inv) in table                             # and under inverses
    flip = {tuple(fwd[g]) for g in (0, 1, 2, 3)}
    for a, b in itertools.product((0, 1, 2, 3), repeat=2):
        assert tuple(fwd[a][fwd[b]]) in flip                   # "flip" is a subgroup


def test_tta_group_names_and_tuples():
    from drs_amd import patches as P
    assert P.tta_group("flip") == (0, 1, 2, 3)
    assert P.tta_group("d4") == tuple(range(8))
    assert P.tta_group((5,)) == (5,)
    assert P.tta_group([3, 0, np.int64(6)]) == (0, 3, 6)        # ascending: the order of the per-pixel sum
    for bad in ("D4", "flips", "", (), (8,), (-1,), (1, 1), (1.0,), (True,), 3, None):
        with pytest.raises(ValueError):
            P.tta_group(bad)


def _check_symmetric_plan(h, w, T, m):
    from drs_amd import patches as P
    boxes = P.dense_tiles(h, w, T, m, m)
    cover = np.zeros((h, w), dtype=np.int32)
    for y0, x0, cy0, cy1, cx0, cx1 in boxes:
        assert 0 <= y0 and y0 + T <= h and 0 <= x0 and x0 + T <= w
        assert y0 <= cy0 < cy1 <= y0 + T and x0 <= cx0 < cx1 <= x0 + T
        # margin m from every tile edge that is not an image border, on both sides of both axes
        assert cy0 == 0 or cy0 - y0 >= m
        assert cy1 == h or y0 + T - cy1 >= m
        assert cx0 == 0 or cx0 - x0 >= m
        assert cx1 == w or x0 + T - cx1 >= m
        cover[cy0:cy1, cx0:cx1] += 1
    assert (cover == 1).all()
    return boxes


def test_symmetric_margin_plan_partitions_and_keeps_the_margin():
    rng = np.random.default_rng(21)
    checked = 0
    while checked < 500:
        h, w = int(rng.integers(1, 140)), int(rng.integers(1, 140))
        b, a = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        m = max(b, a)
        T = int(rng.integers(1, min(h, w) + 1))
        if T < max(h, w) and T <= 2 * m:
            continue
        _check_symmetric_plan(h, w, T, m)
        checked += 1
    # the tests' shapes with Dilated8Pooling's field (50, 51) -> m = 51, and the benchmark's mosaic
    for h, w, T in ((150, 230, 128), (230, 150, 128), (300, 340, 160), (300, 340, 200), (160, 150, 120)):
        _check_symmetric_plan(h, w, T, 51)
    from drs_amd import patches as P
    assert len(P.dense_tiles(6000, 6000, 512, 51, 51)) == 225


def test_cli_dense_tta_flag_parser():
    from drs_amd.cli import parse_dense_tta
    base = ["isprs_dilated_random.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a,b", "c", "0.01", "0.005", "4", "3", "25", "10",
            "dilated8_grsl", "multi_fixed", "9,13", "acc", "generate_final_maps", "--dense-tile=64"]
    got, tta = parse_dense_tta(base)
    assert got == base and got is not base and tta is None
    for pos in (1, 5, len(base)):
        for v in ("flip", "d4"):
            got, tta = parse_dense_tta(base[:pos] + ["--dense-tta=" + v] + base[pos:])
            assert got == base and tta == v, (pos, v)
    for bad in ("--dense-tta", "--dense-tta=", "--dense-tta=D4", "--dense-tta=rot", "--dense-tta=flip,d4", "--dense-tta= d4",
                "--dense-tta=5"):
        with pytest.raises(ValueError):
            parse_dense_tta(base + [bad])
    with pytest.raises(ValueError):
        parse_dense_tta(base + ["--dense-tta=flip", "--dense-tta=flip"])
    for other in ("--dense-ttas", "-dense-tta", "--dense-t"):
        got, tta = parse_dense_tta(base + [other])
        assert got == base + [other] and tta is None


def test_cli_rejects_dense_tta_without_dense_tile_and_bad_values():
    from drs_amd import cli
    from drs_amd.net import NoComm
    argv = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
            "single_fixed", "25", "acc", "generate_final_maps"]
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-tta=d4"], device="cpu", comm=NoComm())
    assert "--dense-tile" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-tile=64", "--dense-tta=rot90"], device="cpu", comm=NoComm())
    assert "flip|d4" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-tile=64", "--dense-tta=d4", "--dense-tta=flip"], device="cpu", comm=NoComm())
    assert "more than once" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv[:-1] + ["training", "--dense-tile=64", "--dense-tta=d4"], device="cpu", comm=NoComm())
    assert "--dense-tile applies" in str(e.value)


def test_loops_reject_tta_without_overlap_tiles():
    from drs_amd import loops
    with pytest.raises(ValueError, match="dense_tile"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, dense_tta="d4")
    with pytest.raises(ValueError, match="dense_tile"):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, dense_tta="flip")
    with pytest.raises(ValueError):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, dense_tile=64, dense_tta="rot")
