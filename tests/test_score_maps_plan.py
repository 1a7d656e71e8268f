"""CPU: the host side of the per-pixel score maps: the names of the maps, the command-line option, and the
calibration scores of a reliability table against values worked out by hand."""
import numpy as np
import pytest

from drs_amd import metrics as MT
from drs_amd import patches as P


# ------------------------------------------------------------------------------------------------------------- the names
def test_score_kinds_are_the_three_maps_of_the_kernel():
    assert P.SCORE_KINDS == ("confidence", "margin", "entropy")


@pytest.mark.parametrize("text, want", [("confidence", ("confidence",)), ("confidence,entropy", ("confidence", "entropy")),
                                        ("entropy,margin,confidence", ("entropy", "margin", "confidence"))])
def test_parse_score_maps_accepts(text, want):
    assert P.parse_score_maps(text) == want


@pytest.mark.parametrize("text", ["", "confidence,", ",entropy", "confidence, entropy", " confidence", "certainty", "confidence,confidence",
                                  "Confidence", "confidence;entropy", "margin,entropy,confidence,margin"])
def test_parse_score_maps_rejects(text):
    with pytest.raises(ValueError) as e:
        P.parse_score_maps(text)
    assert "confidence|margin|entropy" in str(e.value) and repr(text) in str(e.value)


def test_check_score_kinds():
    assert P.check_score_kinds(["margin"]) == ("margin",)
    assert P.check_score_kinds(("entropy", "confidence")) == ("entropy", "confidence")
    for bad in ((), [], "confidence", None, ("confidence", "confidence"), ("sharpness",), 3):
        with pytest.raises(ValueError):
            P.check_score_kinds(bad)


# ------------------------------------------------------------------------------------------------------------- the command line
def test_cli_parse_score_maps_anywhere_in_argv():
    from drs_amd import cli
    argv = ["x.py", "a", "b"]
    assert cli.parse_score_maps(argv) == (argv, None)
    assert cli.parse_score_maps(["x.py", "--score-maps=confidence,margin", "a", "b"]) == (argv, ("confidence", "margin"))
    assert cli.parse_score_maps(argv + ["--score-maps=entropy"]) == (argv, ("entropy",))
    for bad, say in ((["--score-maps"], "confidence,margin,entropy"), (["--score-maps="], "confidence,margin,entropy"),
                     (["--score-maps=loudness"], "confidence,margin,entropy"), (["--score-maps=margin,margin"], "confidence,margin,entropy"),
                     (["--score-maps=margin", "--score-maps=entropy"], "more than once")):
        with pytest.raises(ValueError) as e:
            cli.parse_score_maps(argv + bad)
        assert say in str(e.value)


def test_cli_rejects_score_maps_for_training_and_bad_values():
    from drs_amd import cli
    from drs_amd.net import NoComm
    argv = ["x.py", "synthetic:70x80x5/vaihingen/", "out_", "m", "a", "c", "0.01", "0.005", "4", "3", "25", "10", "dilated8_grsl",
            "single_fixed", "25", "acc"]
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["training", "--score-maps=confidence"], device="cpu", comm=NoComm())
    assert "--score-maps applies to the validate_test and generate_final_maps processes only" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["--score-maps=confidence"] + argv + ["training", "--dense-tile=64"], device="cpu", comm=NoComm())
    assert "applies" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["validate_test", "--score-maps=certainty"], device="cpu", comm=NoComm())
    assert "--score-maps=confidence,margin,entropy" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ["generate_final_maps", "--score-maps=margin", "--score-maps=margin"], device="cpu", comm=NoComm())
    assert "more than once" in str(e.value)


def test_loops_reject_scores_with_return_sums_and_bad_kinds():
    from drs_amd import loops
    with pytest.raises(ValueError, match="return_sums"):
        loops._check_scores(("confidence",), True)
    with pytest.raises(ValueError, match="confidence\\|margin\\|entropy"):
        loops._check_scores(("certainty",), False)
    with pytest.raises(ValueError, match="confidence\\|margin\\|entropy"):
        loops._score_buffers(("certainty",), 4, "cpu")
    assert loops._check_scores(None, True) is None and loops._check_scores(["margin"], False) == ("margin",)
    assert loops._score_buffers(None, 4, "cpu") is None
    bufs = loops._score_buffers(("entropy", "confidence"), 4, "cpu")
    assert list(bufs) == ["entropy", "confidence"] and all(int(v.sum()) == 0 and v.numel() == 4 for v in bufs.values())


# ------------------------------------------------------------------------------------------------------------- calibration
def _table(rows):
    h = np.zeros((256, 2), dtype=np.int64)
    for c, n, right in rows:
        h[c] = (n, right)
    return h


def test_calibration_of_a_perfectly_calibrated_table_is_zero():
    # bytes 51, 102, 204, 255 = confidences 0.2, 0.4, 0.8, 1.0, each right exactly that often; one byte per bin of 15
    cal = MT.calibration(_table([(51, 5, 1), (102, 10, 4), (204, 5, 4), (255, 7, 7)]))
    assert cal["ece"] == pytest.approx(0.0, abs=1e-15) and cal["mce"] == pytest.approx(0.0, abs=1e-15)
    assert cal["count"] == 27
    assert cal["accuracy"] == pytest.approx(16 / 27.0) and cal["mean_confidence"] == pytest.approx(16 / 27.0)
    assert [b["count"] for b in cal["bins"]] == [0, 0, 0, 5, 0, 0, 10, 0, 0, 0, 0, 0, 5, 0, 7]      # 51*15//255 = 3, 6, 12, 14


def test_calibration_all_in_one_bin():
    # 100 pixels at byte 255 (confidence 1), 60 right: every score is the gap 0.4
    cal = MT.calibration(_table([(255, 100, 60)]))
    assert cal["ece"] == pytest.approx(0.4) and cal["mce"] == pytest.approx(0.4)
    assert cal["mean_confidence"] == pytest.approx(1.0) and cal["accuracy"] == pytest.approx(0.6)
    assert len(cal["bins"]) == 15 and cal["bins"][14]["count"] == 100 and sum(b["count"] for b in cal["bins"]) == 100
    assert cal["bins"][14]["lo"] == pytest.approx(14 / 15.0) and cal["bins"][14]["hi"] == pytest.approx(1.0)


def test_calibration_by_hand_two_bins_and_other_bin_counts():
    # bins = 2: bytes 0..127 -> bin 0, 128..255 -> bin 1 (c * 2 // 255; 255 is clamped into the last bin)
    # bin 0: 10 px at byte 51 (0.2), 3 right and 10 px at byte 102 (0.4), 1 right: conf 0.3, acc 0.2, gap 0.1
    # bin 1: 30 px at byte 204 (0.8), 27 right and 10 px at byte 255 (1.0), 9 right: conf 0.85, acc 0.9, gap 0.05
    h = _table([(51, 10, 3), (102, 10, 1), (204, 30, 27), (255, 10, 9)])
    cal = MT.calibration(h, bins=2)
    assert cal["ece"] == pytest.approx((20 * 0.1 + 40 * 0.05) / 60.0) and cal["mce"] == pytest.approx(0.1)
    assert cal["mean_confidence"] == pytest.approx((10 * 0.2 + 10 * 0.4 + 30 * 0.8 + 10 * 1.0) / 60.0)
    assert cal["accuracy"] == pytest.approx(40 / 60.0)
    assert [(b["count"], round(b["confidence"], 12), round(b["accuracy"], 12)) for b in cal["bins"]] == [(20, 0.3, 0.2), (40, 0.85, 0.9)]
    one = MT.calibration(h, bins=1)          # one bin: |accuracy - mean confidence|
    assert one["ece"] == pytest.approx(abs(40 / 60.0 - 40 / 60.0), abs=1e-15)
    full = MT.calibration(h, bins=255)       # a bin per byte (254 and 255 share the last): sum n_c |acc_c - conf_c| / N
    assert full["ece"] == pytest.approx((10 * 0.1 + 10 * 0.3 + 30 * 0.1 + 10 * 0.1) / 60.0)
    assert full["mce"] == pytest.approx(0.3)


def test_calibration_of_an_empty_table():
    cal = MT.calibration(np.zeros((256, 2), dtype=np.int64))
    assert (cal["ece"], cal["mce"], cal["mean_confidence"], cal["accuracy"], cal["count"]) == (0.0, 0.0, 0.0, 0.0, 0)
    assert len(cal["bins"]) == 15 and all(b["count"] == 0 for b in cal["bins"])


def test_calibration_rejects_malformed_tables():
    for bad in (np.zeros((255, 2), dtype=np.int64), np.zeros((256, 2), dtype=np.float64), _table([(3, 1, 2)]), _table([(3, -1, -1)])):
        with pytest.raises(ValueError):
            MT.calibration(bad)
    with pytest.raises(ValueError):
        MT.calibration(np.zeros((256, 2), dtype=np.int64), bins=0)
