"""CPU: overlap-tile inference of squeeze-and-excitation nets with whole-image gates (loops.predict_tile_dense(se="global"), DESIGN.md
8a.3) -- the receptive field with the SE layers taken as constants, the staged algorithm stated in numpy on the fp64 oracle, and the
command line's --dense-se flag."""
import numpy as np
import pytest

from oracle import nets as ON
from oracle import tf_ops as T

CH, K = 5, 6
SE_NET = "dilated_icpr_rate6_SE"


def test_gated_receptive_field_counts_the_se_layers_as_constants():
    from drs_amd import known_net_types, resolve
    from drs_amd.nets import Plan
    # from the oracle's conv specs by the SAME-pad rule (no pools in this net): 2/2, 4/4, 4/5, 6/6, 5/5, 6/6
    pads = [ON.same_pad(k, r) for (_, k, _, _, r) in ON.conv_specs(SE_NET, CH)]
    assert pads == [(2, 2), (4, 4), (4, 5), (6, 6), (5, 5), (6, 6)]
    want = (sum(p[0] for p in pads), sum(p[1] for p in pads))
    assert want == (27, 28)
    plan = Plan(SE_NET, CH, K)
    assert plan.gated_receptive_field == want
    assert plan.receptive_field is None                 # the single-pass field stays undefined
    seen = 0
    for t in sorted({resolve(n) for n in known_net_types()}):
        p = Plan(t, CH, K)
        if p.se:
            assert t == SE_NET
            continue
        assert p.gated_receptive_field == p.receptive_field, t
        seen += 1
    assert seen >= 10


def test_staged_algorithm_on_the_fp64_oracle_equals_its_whole_image_forward():
    """sweep j: every tile forwarded up to the block SE j follows with the gates 0..j-1 as constants, the activated output summed
    over the tile's core; gate j from the mean over all h*w pixels; last sweep: the full forward, core logits placed"""
    from drs_amd import patches as P
    from drs_amd.nets import Plan
    h, w, Tt = 70, 90, 64
    before, after = Plan(SE_NET, CH, K).gated_receptive_field
    boxes = P.dense_tiles(h, w, Tt, before, after)
    assert len(boxes) >= 4
    rng = np.random.default_rng(0)
    o = T.OracleNet(SE_NET, CH, K, seed=4)
    for (name, _, _, co, _) in o.convs:
        o.p[name + "/moving_mean"] = rng.normal(size=co) * 0.1
        o.p[name + "/moving_variance"] = rng.uniform(0.5, 2.0, size=co)
    for sc in o.spec["se"].values():        # gates far from the constant sigmoid(0.1) of the initialiser
        for fc in ("_fc1", "_fc2"):
            o.p[sc + fc + "/weights"] = rng.normal(size=o.p[sc + fc + "/weights"].shape) * 0.3
    x = rng.normal(size=(h, w, CH))
    ref = o.forward(x[None], False)[0]
    se_at = sorted(o.spec["se"])

    def chain(tile, gates, stop):
        """blocks 0..stop of one tile with the given gates as constants; the activated (ungated) output of block `stop`"""
        cur = tile[None]
        for li in range(stop + 1):
            cur = o._block_fwd(li, cur, False, None)
            if li in o.spec["se"] and li != stop:
                cur = cur * gates[se_at.index(li)]
        return cur[0]

    o._cache = {}
    gates = []
    for j, li in enumerate(se_at):
        C = o.convs[li][3]
        sums = np.zeros(C)
        seen = np.zeros((h, w), dtype=np.int64)
        for (y0, x0, cy0, cy1, cx0, cx1) in boxes:
            a = chain(x[y0:y0 + Tt, x0:x0 + Tt], gates, li)
            sums += a[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0].sum(axis=(0, 1))
            seen[cy0:cy1, cx0:cx1] += 1
        assert (seen == 1).all()            # cores partition the image: every pixel counted once
        s = sums / (h * w)
        sc = o.spec["se"][li]
        e1 = np.maximum(s @ o.p[sc + "_fc1/weights"] + o.p[sc + "_fc1/biases"], 0)
        gates.append(1.0 / (1.0 + np.exp(-(e1 @ o.p[sc + "_fc2/weights"] + o.p[sc + "_fc2/biases"]))))
    assert max(np.ptp(g) for g in gates) > 1e-3
    got = np.zeros((h, w, K))
    last = se_at[-1]
    for (y0, x0, cy0, cy1, cx0, cx1) in boxes:
        feat = chain(x[y0:y0 + Tt, x0:x0 + Tt], gates, last) * gates[-1]
        lg = feat @ o.p["conv_classifier/weights"][0, 0] + o.p["conv_classifier/biases"]
        got[cy0:cy1, cx0:cx1] = lg[cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0]
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= 1e-10, err
    # and the window-style gate (each tile's own mean) is a different function: the mode cannot be a silent default
    own = o.forward(x[None, :Tt, :Tt], False)[0]
    assert np.abs(own[:20, :20] - ref[:20, :20]).max() / np.abs(ref).max() > 1e-6


def test_core_boxes_in_transformed_tiles_and_why_every_code_has_gates_of_its_own():
    from drs_amd import patches as P
    h, w, Tt = 150, 230, 128
    bx = P.dense_tiles(h, w, Tt, 28, 28)
    for g in range(8):
        for (y0, x0, a, b, c, d), l in zip(bx, P.dihedral_core_boxes(bx, Tt, g)):
            m = np.zeros((Tt, Tt), dtype=bool)
            m[a - y0:b - y0, c - x0:d - x0] = True
            m2 = np.zeros((Tt, Tt), dtype=bool)
            m2[l[2]:l[3], l[4]:l[5]] = True
            assert l[0] == 0 and l[1] == 0 and (P.dihedral_apply(m, g) == m2).all(), g
    # the net is not equivariant: the first SE block's input mean of a transposed image is not that of the image (fp64 oracle)
    rng = np.random.default_rng(3)
    o = T.OracleNet(SE_NET, CH, K, seed=4)
    x = rng.normal(size=(40, 56, CH))
    means = []
    for g in (0, 4):
        o.forward(np.ascontiguousarray(P.dihedral_apply(x, g))[None], False)
        means.append(o._se_cache[1][1][0][0])
    assert np.abs(means[0] - means[1]).max() / np.abs(means[0]).max() > 1e-4


def test_cli_dense_se_flag_parser():
    from drs_amd.cli import parse_dense_se
    base = ["isprs_dilated_random.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a,b", "c", "0.01", "0.005", "4", "3", "25", "10",
            SE_NET, "multi_fixed", "9,13", "acc", "generate_final_maps", "--dense-tile=64"]
    got, se = parse_dense_se(base)
    assert got == base and got is not base and se is None
    for pos in (1, 5, len(base)):
        got, se = parse_dense_se(base[:pos] + ["--dense-se=global"] + base[pos:])
        assert got == base and se == "global", pos
    for bad in ("--dense-se", "--dense-se=", "--dense-se=Global", "--dense-se=local", "--dense-se=global,global", "--dense-se= global"):
        with pytest.raises(ValueError):
            parse_dense_se(base + [bad])
    with pytest.raises(ValueError):
        parse_dense_se(base + ["--dense-se=global", "--dense-se=global"])
    for other in ("--dense-ses", "-dense-se", "--dense-s"):
        got, se = parse_dense_se(base + [other])
        assert got == base + [other] and se is None


def test_cli_and_loops_reject_dense_se_without_dense_tile_and_bad_values():
    from drs_amd import cli, loops
    from drs_amd.net import NoComm
    argv = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", SE_NET,
            "single_fixed", "25", "acc", "generate_final_maps"]
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-se=global"], device="cpu", comm=NoComm())
    assert "--dense-tile" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-tile=64", "--dense-se=window"], device="cpu", comm=NoComm())
    assert "--dense-se=global" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["--dense-tile=64", "--dense-se=global", "--dense-se=global"], device="cpu", comm=NoComm())
    assert "more than once" in str(e.value)
    with pytest.raises(ValueError, match="dense_tile"):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, dense_se="global")
    with pytest.raises(ValueError, match="dense_tile"):
        loops.generate_final_maps(None, [], [], 1, None, None, "acc", "single_fixed", [25], "vaihingen", None, dense_se="global")
    with pytest.raises(ValueError):
        loops.validate_test(None, [], [], [], 1, None, None, 25, 0, dense_tile=64, dense_se="local")
