"""CPU: the argument-domain contract of the op-level C ABI (include/drs.h, "Ranges, else DRS_ERR_ARG").

One table row per entry point that launches a kernel: a baseline call inside the domain and a list of single-argument violations,
one for every bound the header states, every pointer that must not be NULL, and NaN / inf for the float parameters that have a
range.  Argument validation is host code that runs before the first HIP call, so the raw ctypes functions are called with dummy
device pointers (HOST-pointer arguments get real ctypes arrays) and the return code is compared:
  - every violation returns exactly DRS_ERR_ARG;
  - the baseline does not (without a device it comes back as DRS_ERR_HIP from the launch), so each rejection is the doing of the one
    changed argument.
On a machine with a GPU a baseline -- or a row whose check were missing -- would launch on the dummy pointers: the module skips itself
there.  A meta-test parses include/drs.h and requires every op-level `int drs_*(` / `size_t drs_*(` declaration to have a row or to
stand on the list of exclusions below with its reason."""
import ctypes as C
import os
import re

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("the baseline rows would launch kernels on dummy pointers: CPU machines only", allow_module_level=True)

from drs_amd import _lib  # noqa: E402

OK, ERR_ARG, ERR_HIP = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

# dummy device pointers (never dereferenced by host code), 256-byte aligned as an allocator's are
D = [0x10000 + 0x1000 * i for i in range(32)]
p0, p1, p2, p3, p4, p5, p6, p7, p8, p9, p10, p11, p12 = D[:13]

# HOST-pointer arguments (the header marks them): real memory
MEAN3 = (C.c_double * 3)(0.3, 0.4, 0.5)
STD3 = (C.c_double * 3)(0.1, 0.2, 0.3)
WEIGHTS = (C.c_float * 6)(1.0, 2.0, 0.5, 1.0, 1.5, 0.25)
W_NEG = (C.c_float * 6)(1.0, -2.0, 0.5, 1.0, 1.5, 0.25)
W_NAN = (C.c_float * 6)(1.0, 2.0, NAN, 1.0, 1.5, 0.25)
W_INF = (C.c_float * 6)(1.0, 2.0, 0.5, INF, 1.5, 0.25)
DIST = (C.c_int * 3)(1, 3, 5)
DIST_EQ = (C.c_int * 3)(1, 3, 3)
DIST_DESC = (C.c_int * 3)(1, 5, 3)
DIST_ZERO = (C.c_int * 3)(0, 3, 5)
DIST_FAR = (C.c_int * 3)(1, 3, 17)
EXECUTED, TOTAL = (C.c_longlong * 1)(), (C.c_longlong * 1)()

ROWS = {}


def row(name, args, bad, optional=()):
    """args: ordered (name, baseline value) pairs without the trailing stream; bad: dicts of the one (rarely two: a pair that is
    only wrong together) argument changed; optional: pointer arguments that may be NULL.  A NULL violation is added for every other
    pointer argument of the baseline."""
    assert name not in ROWS, name
    names = [k for k, _ in args]
    assert len(set(names)) == len(names), name
    ptrs = [k for k, v in args if (isinstance(v, int) and v in D) or isinstance(v, C.Array)]
    nulls = [{k: None} for k in ptrs if k not in optional]
    ROWS[name] = (args, list(bad) + nulls)


# ------------------------------------------------------------------------------------------------------------- convolutions
CONV = [("in", p0), ("B", 2), ("S", 9), ("P", 2), ("ld_in", 64), ("coff_in", 32), ("w", p1), ("bias", p2), ("k", 3), ("rate", 2),
        ("pad_before", 2), ("cin", 32), ("cout", 64), ("out", p3), ("ld_out", 96), ("coff_out", 32), ("accumulate", 0),
        ("stats_partial", None)]
CONV_BAD = [dict(B=0), dict(S=0), dict(S=-9), dict(B=1 << 12, S=64), dict(k=0), dict(rate=0), dict(cin=0), dict(cin=24), dict(cin=-32),
            dict(cout=0), dict(cout=48), dict(cout=-64), dict(pad_before=-1), dict(pad_before=3), dict(P=1), dict(pad_before=1),
            dict(coff_in=-32), dict(coff_in=33), dict(ld_in=63), dict(ld_in=32), dict(coff_out=-1), dict(coff_out=33), dict(ld_out=95),
            dict(accumulate=1, stats_partial=p4), dict(B=8, S=100, P=100, ld_in=2048, coff_in=0), dict(k=1 << 15, P=1 << 17)]
CONV8_BAD = [dict(cin=8, ld_in=10, coff_in=0), dict(cin=8, ld_in=12, coff_in=2), dict(cin=16, ld_in=18, coff_in=0)]
row("drs_conv_forward", CONV, CONV_BAD + CONV8_BAD, optional=("bias",))
row("drs_conv_forward_ws", CONV + [("workspace", None), ("workspace_floats", 0)], CONV_BAD + CONV8_BAD, optional=("bias",))
row("drs_conv_executed_ksteps", [("B", 2), ("S", 9), ("k", 3), ("rate", 2), ("pad_before", 2), ("cin", 32), ("cout", 64),
                                 ("executed", EXECUTED), ("total", TOTAL)],
    [dict(B=0), dict(S=0), dict(S=-9), dict(B=1 << 12, S=64), dict(k=0), dict(rate=0), dict(cin=0), dict(cout=0), dict(cout=48)])

WGRAD = [("x", p0), ("B", 2), ("S", 9), ("Px", 2), ("ld_x", 64), ("coff_x", 32), ("g", p1), ("Pg", 5), ("ld_g", 96), ("coff_g", 32),
         ("k", 3), ("rate", 2), ("pad_before", 2), ("cin", 32), ("cin_real", 32), ("cout", 64), ("slab", p2), ("grad", p3)]
WGRAD_BAD = [dict(B=0), dict(S=0), dict(S=-9), dict(B=1 << 12, S=64), dict(k=0), dict(rate=0), dict(cin=0), dict(cin=24), dict(cout=0),
             dict(cout=48), dict(cin_real=0), dict(cin_real=33), dict(pad_before=-1),
             dict(Px=1), dict(Px=0), dict(pad_before=1), dict(pad_before=3),           # the halo of x against pad_before and pad_after
             dict(Pg=-1), dict(coff_x=-32), dict(coff_x=64), dict(ld_x=32), dict(coff_g=-32), dict(coff_g=64), dict(ld_g=64)]
G_SLAB = dict(B=8, S=100, Pg=100, ld_g=2048, coff_g=0)       # 2^30 floats and more (with two terms: 2^31 and more)
row("drs_conv_wgrad", WGRAD, WGRAD_BAD + [dict(cin=8, cin_real=5, ld_x=10, coff_x=0), dict(cin=8, cin_real=5, ld_x=12, coff_x=2),
                                          dict(coff_x=33), dict(ld_g=95), dict(B=8, S=100, Px=100, ld_x=2048, coff_x=0), G_SLAB])
row("drs_conv_wgrad_split", WGRAD + [("nterms", 2)],
    WGRAD_BAD + [dict(nterms=1), dict(nterms=4), dict(cout=32), dict(cout=96), dict(ld_x=80), dict(coff_x=16), dict(ld_g=112),
                 dict(coff_g=16), dict(B=8, S=100, Px=150, ld_x=2048, coff_x=0), G_SLAB])      # x: 2^32 term elements and more
row("drs_filter_flip_transpose", [("w", p0), ("wt", p1), ("k", 3), ("cin", 32), ("cout", 64)],
    [dict(k=0), dict(k=-3), dict(cin=0), dict(cin=-32), dict(cout=0), dict(cout=-64), dict(k=1 << 12, cin=256)])
row("drs_filter_pad_cin", [("w", p0), ("wp", p1), ("k", 3), ("cin", 5), ("cin_pad", 8), ("cout", 64)],
    [dict(k=0), dict(cin=0), dict(cin=-5), dict(cin_pad=4), dict(cout=0), dict(cout=-64), dict(k=1 << 12, cin_pad=256)])
row("drs_split_terms", [("src", p0), ("n", 64), ("nterms", 2), ("terms", p1)], [dict(n=48), dict(nterms=1), dict(nterms=4)])
row("drs_filter_split", [("w", p0), ("k", 3), ("cin", 32), ("cin_pad", 32), ("cout", 64), ("nterms", 2), ("wf", p1), ("wd", p2)],
    [dict(k=0), dict(cin=0), dict(cin_pad=0), dict(cin_pad=48), dict(cin=33), dict(cin=5), dict(cout=0), dict(cout=48), dict(nterms=1),
     dict(nterms=4), dict(k=1 << 12, cin_pad=256)], optional=("wd",))
row("drs_conv_forward_split", CONV + [("nterms", 2)],
    [b for b in CONV_BAD if b not in (dict(coff_in=33), dict(ld_in=63))] +
    [dict(nterms=1), dict(nterms=4), dict(cout=32), dict(cout=96), dict(cin=8, ld_in=32, coff_in=0), dict(ld_in=80), dict(coff_in=16),
     dict(ld_in=48, coff_in=32)], optional=("bias",))

# ------------------------------------------------------------------------------------------------------------- batch norm
row("drs_stats_reduce", [("partial", p0), ("nrows", 7), ("C", 64), ("sums", p1), ("scratch", None)], [dict(nrows=0), dict(C=0)])
row("drs_stats_reduce_means", [("partial", p0), ("nrows", 7), ("C", 64), ("count", 162.0), ("sums", None), ("means", p1)],
    [dict(nrows=0), dict(C=0), dict(count=0.5), dict(count=-1.0), dict(count=NAN), dict(count=INF)])
row("drs_conv_stats_reduce", [("partial", p0), ("M", 162), ("mtile", 128), ("C", 64), ("sums", p1), ("scratch", None)],
    [dict(M=0), dict(mtile=0), dict(C=0)])
row("drs_conv_stats_finish", [("partial", p0), ("M", 162), ("mtile", 128), ("C", 64), ("count", 162.0), ("mean_rstd", p1),
                              ("moving_mean", p2), ("moving_var", p3), ("decay", 0.999), ("bessel", 1), ("sums", None)],
    [dict(M=0), dict(mtile=0), dict(C=0), dict(count=0.0), dict(count=NAN), dict(count=INF), dict(decay=-0.1), dict(decay=1.5),
     dict(decay=NAN), dict(decay=INF), dict(moving_mean=None), dict(moving_var=None)], optional=("moving_mean", "moving_var"))
row("drs_bn_finish", [("sums", p0), ("count", 162.0), ("C", 64), ("mean_rstd", p1), ("moving_mean", p2), ("moving_var", p3),
                      ("decay", 0.999), ("bessel", 1)],
    [dict(C=0), dict(C=-4), dict(count=0.0), dict(count=NAN), dict(count=INF), dict(decay=-0.1), dict(decay=1.5), dict(decay=NAN),
     dict(decay=INF), dict(moving_mean=None), dict(moving_var=None)], optional=("moving_mean", "moving_var"))
row("drs_bn_eval_coeffs", [("moving_mean", p0), ("moving_var", p1), ("C", 64), ("mean_rstd", p2)], [dict(C=0), dict(C=-4)])

VIEW_BAD = [dict(B=0), dict(S=0), dict(S=-9), dict(B=8192, S=9), dict(B=4, S=2048), dict(C=0), dict(C=-4), dict(C=30)]
OUT_BAD = [dict(P_out=-1), dict(B=6000, S=9, P_out=1), dict(coff_out=-4), dict(coff_out=36), dict(ld_out=92), dict(coff_out=34),
           dict(ld_out=98), dict(ld_out=60, coff_out=0)]
ALPHA_BAD = [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=NAN), dict(alpha=INF)]
COUNT_BAD = [dict(count=0.0), dict(count=NAN), dict(count=INF)]
BNF = [("z", p0), ("B", 2), ("S", 9), ("C", 64), ("mean_rstd", p1), ("alpha", 0.1), ("pool", 1), ("out", p2), ("P_out", 2),
       ("ld_out", 96), ("coff_out", 32), ("argmax", p3)]
row("drs_bn_act_pool_forward", BNF, VIEW_BAD + OUT_BAD + ALPHA_BAD, optional=("argmax",))
row("drs_bn_finish_act_pool_forward",
    [("sums", p4), ("count", 162.0), ("mean_rstd", p1), ("moving_mean", p5), ("moving_var", p6), ("decay", 0.999), ("bessel", 1),
     ("z", p0), ("B", 2), ("S", 9), ("C", 64), ("alpha", 0.1), ("pool", 1), ("out", p2), ("P_out", 2), ("ld_out", 96), ("coff_out", 32),
     ("argmax", p3)],
    VIEW_BAD + OUT_BAD + ALPHA_BAD + COUNT_BAD + [dict(decay=-0.1), dict(decay=1.5), dict(decay=NAN), dict(pool=0), dict(pool=2),
                                                  dict(C=516, ld_out=1024), dict(moving_mean=None), dict(moving_var=None)],
    optional=("argmax", "moving_mean", "moving_var"))
row("drs_bn_act_pool_forward_terms", BNF + [("terms", p4), ("nterms", 2)],
    VIEW_BAD + [b for b in OUT_BAD if b != dict(coff_out=36)] + ALPHA_BAD +
    [dict(nterms=1), dict(nterms=4), dict(coff_out=16, ld_out=96), dict(ld_out=112), dict(out=None, terms=None)],
    optional=("argmax", "out"))
row("drs_bn_backward_reduce",
    [("ga", p0), ("ld_ga", 96), ("coff_ga", 32), ("z", p1), ("argmax", p2), ("B", 2), ("S", 9), ("C", 64), ("mean_rstd", p3),
     ("alpha", 0.1), ("pool", 1), ("gxhat", p4), ("partial", p5)],
    VIEW_BAD + ALPHA_BAD + [dict(C=1028, ld_ga=2048), dict(coff_ga=-4), dict(coff_ga=36), dict(ld_ga=92), dict(coff_ga=34), dict(ld_ga=98)])
BNB = [("gxhat", p0), ("z", p1), ("B", 2), ("S", 9), ("C", 64), ("mean_rstd", p2), ("sums", p3), ("count", 162.0), ("gz", p4),
       ("P_out", 2), ("ld_out", 96), ("coff_out", 32)]
row("drs_bn_backward_apply", BNB, VIEW_BAD + OUT_BAD + COUNT_BAD + [dict(C=1028, ld_out=2048)])
row("drs_bn_backward_apply_means", [a for a in BNB if a[0] != "count"][:6] + [("means", p3)] + BNB[8:],
    VIEW_BAD + OUT_BAD + [dict(C=1028, ld_out=2048)])
row("drs_bn_backward_apply_terms", BNB + [("terms", p5), ("nterms", 3)],
    VIEW_BAD + [b for b in OUT_BAD if b != dict(coff_out=36)] + COUNT_BAD +
    [dict(C=1028, ld_out=2048), dict(nterms=1), dict(nterms=4), dict(coff_out=16), dict(ld_out=112), dict(gz=None, terms=None)],
    optional=("gz",))

# ------------------------------------------------------------------------------------------------------------- pools, SE
G_BAD = [dict(coff_g=-4), dict(coff_g=36), dict(ld_g=92), dict(coff_g=34), dict(ld_g=98)]
row("drs_avg_pool_forward", [("in", p0), ("B", 2), ("S", 9), ("C", 64), ("k", 3), ("out", p1), ("P_out", 2), ("ld_out", 96),
                             ("coff_out", 32)], VIEW_BAD + OUT_BAD + [dict(k=0), dict(k=2), dict(k=-3)])
row("drs_avg_pool_backward", [("gout", p0), ("ld_g", 96), ("coff_g", 32), ("B", 2), ("S", 9), ("C", 64), ("k", 3), ("gin", p1)],
    VIEW_BAD + G_BAD + [dict(k=0), dict(k=2), dict(k=-3)])
row("drs_se_forward",
    [("act", p0), ("B", 2), ("S", 9), ("C", 64), ("R", 16), ("w1", p1), ("b1", p2), ("w2", p3), ("b2", p4), ("s", p5), ("e1", p6),
     ("e2", p7), ("out", p8), ("P_out", 2), ("ld_out", 96), ("coff_out", 32)],
    VIEW_BAD + OUT_BAD + [dict(R=0), dict(R=-16), dict(R=16384)])
row("drs_se_backward",
    [("gy", p0), ("ld_g", 96), ("coff_g", 32), ("act", p1), ("s", p2), ("e1", p3), ("e2", p4), ("w1", p5), ("w2", p6), ("B", 2), ("S", 9),
     ("C", 64), ("R", 16), ("gact", p7), ("dw1", p8), ("db1", p9), ("dw2", p10), ("db2", p11), ("scratch", p12)],
    VIEW_BAD + G_BAD + [dict(R=0), dict(R=-16), dict(R=16384)])
row("drs_se_core_sums", [("act", p0), ("C", 64), ("T", 32), ("boxes", p1), ("n", 4), ("sums", p2), ("scratch", p3)],
    [dict(C=0), dict(T=0), dict(T=65536), dict(n=0), dict(n=65536), dict(T=4096, n=128)])
row("drs_se_gate", [("sums", p0), ("count", 2080.0), ("C", 64), ("R", 16), ("w1", p1), ("b1", p2), ("w2", p3), ("b2", p4), ("s", p5),
                    ("e1", p6), ("e2", p7)],
    [dict(C=0), dict(R=0), dict(R=16384), dict(count=0.0), dict(count=-1.0), dict(count=NAN), dict(count=INF)])
row("drs_se_scale_const", [("act", p0), ("B", 2), ("S", 9), ("C", 64), ("e2", p1), ("out", p2), ("P_out", 2), ("ld_out", 96),
                           ("coff_out", 32)], VIEW_BAD + OUT_BAD)

# ------------------------------------------------------------------------------------------------------------- classifier, reductions
CLS_HEAD = [("feat", p0), ("B", 2), ("S", 9), ("P", 1), ("ld", 96), ("coff", 32), ("C", 64), ("K", 6), ("w", p1), ("bias", p2),
            ("labels", p3), ("loss_mask", p4), ("acc_mask", p5), ("inv_n", 1.0 / 162)]
CLS_TAIL = [("logits", p6), ("pred", p7), ("gfeat", p8), ("ld_g", 96), ("coff_g", 32), ("dw_partial", p9), ("db_partial", p10),
            ("loss_partial", p11), ("conf", p12)]
CLS_OPT = ("labels", "loss_mask", "acc_mask", "logits", "pred", "gfeat", "dw_partial", "db_partial", "loss_partial", "conf",
           "class_weights")
CLS_BAD = [dict(B=0), dict(S=0), dict(S=-9), dict(B=1 << 12, S=64), dict(P=-1), dict(C=0), dict(C=32), dict(C=96), dict(C=512, ld=1024),
           dict(K=0), dict(K=9), dict(inv_n=-1.0), dict(inv_n=NAN), dict(inv_n=INF), dict(coff=-4), dict(coff=34), dict(coff=36),
           dict(ld=92), dict(ld=98), dict(coff_g=-4), dict(coff_g=34), dict(coff_g=36), dict(ld_g=92), dict(ld_g=98),
           dict(loss_partial=None), dict(dw_partial=None), dict(db_partial=None), dict(labels=None),     # each needed by what is still given
           dict(B=8, S=100, P=100, ld=2048, coff=0)]
row("drs_classifier_loss", CLS_HEAD + CLS_TAIL, CLS_BAD, optional=CLS_OPT)
row("drs_classifier_loss_weighted", CLS_HEAD + [("class_weights", WEIGHTS)] + CLS_TAIL,
    CLS_BAD + [dict(class_weights=W_NEG), dict(class_weights=W_NAN), dict(class_weights=W_INF)], optional=CLS_OPT)
row("drs_classifier_loss_focal", CLS_HEAD + [("class_weights", WEIGHTS), ("focal_gamma", 2.0)] + CLS_TAIL,
    CLS_BAD + [dict(class_weights=W_NEG), dict(class_weights=W_NAN), dict(class_weights=W_INF), dict(focal_gamma=-1.0),
               dict(focal_gamma=8.5), dict(focal_gamma=NAN), dict(focal_gamma=INF)], optional=CLS_OPT)
row("drs_label_histogram", [("labels", p0), ("n", 1000), ("K", 6), ("void_label", -1), ("counts", p1)],
    [dict(n=0), dict(n=1 << 40), dict(K=0), dict(K=9)])
row("drs_reliability_histogram", [("truth", p0), ("pred", p1), ("confidence", p2), ("n", 1000), ("K", 6), ("ignore_label", -1),
                                  ("hist", p3)], [dict(n=0), dict(n=1 << 40), dict(K=0), dict(K=9)])
row("drs_temperature_stats", [("sums", p0), ("occur", p1), ("truth", p2), ("n", 1000), ("K", 6), ("sums_are_prob", 0),
                              ("ignore_label", -1), ("beta", 1.5), ("scratch", p3), ("out", p4)],
    [dict(n=1 << 40), dict(K=0), dict(K=9), dict(beta=0.0), dict(beta=1.0 / 128), dict(beta=65.0), dict(beta=-1.0), dict(beta=NAN),
     dict(beta=INF)])
row("drs_rows_reduce_f32", [("in", p0), ("nrows", 3), ("ncols", 384), ("out", p1), ("scratch", p2)],
    [dict(nrows=0), dict(ncols=0), dict(ncols=-1)])
row("drs_sum_f64", [("in", p0), ("n", 3), ("out", p1)], [dict(n=0), dict(n=-1)])
row("drs_scale_f64", [("x", p0), ("n", 3), ("s", 0.5)], [dict(n=0), dict(n=-1)])
row("drs_l2_loss", [("w", p0), ("n", 1000), ("scratch", p1), ("out", p2)], [dict(n=0), dict(n=1 << 40), dict(n=2 ** 64 - 1)])
row("drs_momentum_update", [("w", p0), ("grad", p1), ("accum", p2), ("n", 1000), ("n_decay", 900), ("lr", 0.01), ("weight_decay", 0.005),
                            ("momentum", 0.9), ("grad_scale", 1.0)],
    [dict(n=0), dict(n=1 << 40), dict(n_decay=1001), dict(n_decay=2 ** 64 - 1)])
row("drs_confusion", [("labels", p0), ("pred", p1), ("mask", p2), ("n", 1000), ("K", 6), ("ignore_label", -1), ("conf", p3)],
    [dict(n=0), dict(n=1 << 32), dict(n=2 ** 64 - 1), dict(K=0), dict(K=9)], optional=("mask",))

# ------------------------------------------------------------------------------------------------------------- crops
CROP = [("tiles", p0), ("tiles_are_f64", 1), ("labels", p1), ("tile_off", p2), ("lab_off", p3), ("tile_h", p4), ("tile_w", p5)]
CROP_TAIL = [("rot", p7), ("rot_on", p8), ("noise", None), ("noise_on", p9), ("seed", 7), ("noise_index0", 0), ("mean3", MEAN3),
             ("std3", STD3), ("B", 2), ("S", 9), ("P", 2), ("ld", 8), ("out", p10), ("out_lab", p11), ("out_mask", p12),
             ("void_label", -1), ("quantize_f16", 0)]
CROP_OPT = ("rot", "rot_on", "noise", "noise_on", "out_lab", "out_mask")
CROP_BAD = [dict(C=0), dict(C=9), dict(ld=4), dict(ld=10), dict(B=0), dict(S=0), dict(S=-9), dict(P=-1), dict(B=6000, S=9, P=1),
            dict(noise_index0=-1), dict(quantize_f16=-1), dict(quantize_f16=3)]
row("drs_crop_normalize", CROP + [("C", 5), ("inst", p6)] + CROP_TAIL, CROP_BAD, optional=CROP_OPT)
row("drs_crop_normalize_scaled", CROP + [("n_maps", 3), ("C", 5), ("inst", p6), ("geo", D[13])] + CROP_TAIL,
    CROP_BAD + [dict(n_maps=0)], optional=CROP_OPT)
TILES = [("tiles", p0), ("tiles_are_f64", 1), ("tile_off", p2), ("tile_h", p4), ("tile_w", p5), ("n_maps", 3), ("C", 5), ("inst", p6)]
TILES_TAIL = [("g", 5), ("mean3", MEAN3), ("std3", STD3), ("B", 2), ("T", 32), ("P", 2), ("ld", 8), ("out", p10)]
TILES_BAD = [dict(n_maps=0), dict(C=0), dict(C=9), dict(ld=4), dict(ld=10), dict(g=-1), dict(g=8), dict(B=0), dict(T=0), dict(P=-1),
             dict(B=2000, T=32, P=1)]
row("drs_crop_dihedral", TILES + TILES_TAIL, TILES_BAD)
row("drs_crop_resampled", TILES + [("hs", 60), ("ws", 70)] + TILES_TAIL, TILES_BAD + [dict(hs=0), dict(ws=0)])

# ------------------------------------------------------------------------------------------------------------- whole-map inference
STITCH = [("prob", p0), ("occur", p1), ("logits", p2), ("h", 70), ("w", 57), ("K", 6), ("S", 25), ("stride", 5), ("first_window", 0),
          ("n_windows", 7)]
row("drs_stitch_accumulate", STITCH,
    [dict(h=64, w=64, S=16, stride=2), dict(h=70, w=70, S=25, stride=4), dict(h=56, w=56, S=26, stride=5),      # more than 5 regular windows
     dict(stride=0), dict(stride=-5), dict(S=0), dict(S=-25), dict(h=0), dict(w=0), dict(h=24), dict(w=24), dict(K=0), dict(K=9),
     dict(first_window=-1), dict(n_windows=0), dict(first_window=10 * 8), dict(n_windows=10 * 8 + 1),
     dict(h=70000, w=70000, S=20000, stride=5000, n_windows=121),          # more than 65535 image rows in one call
     dict(h=1 << 20, w=1 << 20, S=5, stride=1)])                            # a window grid of 2^40
# inside the domain: 5 regular windows on one axis, 5 plus the shifted one on the other; and the ordinary half-side stride
STITCH_OK = [dict(h=70, w=57, S=25, stride=5), dict(h=64, w=64, S=16, stride=8)]
row("drs_stitch_finalize", [("prob", p0), ("occur", p1), ("h", 40), ("w", 52), ("K", 6), ("out", p2)],
    [dict(h=0), dict(w=0), dict(h=-40), dict(K=0), dict(K=9)])
row("drs_softmax_accumulate", [("prob", p0), ("occur", p1), ("h", 40), ("w", 52), ("K", 6), ("acc", p2)],
    [dict(h=0), dict(w=0), dict(w=-52), dict(K=0), dict(K=9)])
PLACE = [("prob", p0), ("occur", p1), ("logits", p2), ("h", 40), ("w", 52), ("K", 6), ("T", 32), ("boxes", p3), ("n", 4)]
PLACE_BAD = [dict(K=0), dict(K=9), dict(T=0), dict(T=41), dict(h=31), dict(w=31), dict(n=0), dict(n=65536),
             dict(h=70000, w=70000, T=65536)]
row("drs_tile_place", PLACE, PLACE_BAD)
row("drs_tile_place_dihedral", PLACE + [("g", 5)], PLACE_BAD + [dict(g=-1), dict(g=8)])
row("drs_resample_accumulate", [("src", p0), ("occur", p1), ("hs", 30), ("ws", 39), ("K", 6), ("src_is_prob", 0), ("h", 40), ("w", 52),
                                ("acc", p2)],
    [dict(hs=0), dict(ws=0), dict(h=0), dict(w=0), dict(h=65536), dict(K=0), dict(K=9)])
SCORES = [("sums", p0), ("occur", p1), ("h", 40), ("w", 52), ("K", 6), ("sums_are_prob", 0)]
SCORE_OUT = [("labels", p2), ("confidence", p3), ("margin", p4), ("entropy", p5)]
SCORES_BAD = [dict(h=0), dict(w=0), dict(K=0), dict(K=9), dict(labels=None, confidence=None, margin=None, entropy=None)]
row("drs_stitch_finalize_scores", SCORES + SCORE_OUT, SCORES_BAD, optional=("labels", "confidence", "margin", "entropy"))
row("drs_stitch_finalize_scores_t", SCORES + [("beta", 1.5)] + SCORE_OUT,
    SCORES_BAD + [dict(beta=0.0), dict(beta=1.0 / 128), dict(beta=65.0), dict(beta=NAN), dict(beta=INF)],
    optional=("labels", "confidence", "margin", "entropy"))
row("drs_crf_unary", [("sums", p0), ("occur", p1), ("h", 40), ("w", 52), ("K", 6), ("sums_are_prob", 0), ("beta", 1.5), ("logp", p2),
                      ("q0", p3), ("live", p4)],
    [dict(h=0), dict(w=0), dict(K=1), dict(K=9), dict(beta=0.0), dict(beta=65.0), dict(beta=NAN), dict(beta=INF)])
row("drs_crf_step",
    [("q_in", p0), ("logp", p1), ("live", p2), ("tile", p3), ("tile_is_f64", 1), ("C", 5), ("h", 40), ("w", 50), ("K", 6), ("row0", 0),
     ("rows", 40), ("R", 5), ("step", 2), ("w_app", 4.0), ("theta_xy", 8.0), ("theta_rgb", 0.08), ("w_smooth", 2.0), ("theta_s", 2.0),
     ("q_out", p4)],
    [dict(K=1), dict(K=9), dict(C=0), dict(C=9), dict(R=0), dict(R=7), dict(step=0), dict(step=5), dict(R=5, step=3), dict(R=4, step=4),
     dict(w_app=-1.0), dict(w_app=NAN), dict(w_app=INF), dict(w_smooth=-1.0), dict(w_smooth=NAN), dict(w_smooth=INF),
     dict(theta_xy=0.0), dict(theta_xy=NAN), dict(theta_xy=INF), dict(theta_rgb=0.0), dict(theta_rgb=-0.08), dict(theta_rgb=1e-30),
     dict(theta_rgb=NAN), dict(theta_rgb=INF), dict(theta_s=0.0), dict(theta_s=NAN), dict(theta_s=INF),
     dict(row0=-1), dict(rows=0), dict(row0=1), dict(rows=41), dict(h=0), dict(w=0), dict(q_out=p0)])
row("drs_boundary_distance", [("map", p0), ("h", 40), ("w", 52), ("R", 5), ("d2", p1)],
    [dict(h=0), dict(w=0), dict(h=1 << 20, w=1 << 20), dict(R=0), dict(R=17)])
row("drs_boundary_histogram", [("truth", p0), ("pred", p1), ("h", 40), ("w", 52), ("K", 6), ("ignore_label", -1), ("distances", DIST),
                               ("n", 3), ("hist", p2)],
    [dict(h=0), dict(w=0), dict(h=1 << 20, w=1 << 20), dict(K=1), dict(K=9), dict(n=0), dict(n=9), dict(distances=DIST_EQ),
     dict(distances=DIST_DESC), dict(distances=DIST_ZERO), dict(distances=DIST_FAR)])

# op-level declarations without a row: they launch nothing and cannot reject anything
EXCLUDED = {
    "drs_conv_mtile": "pure size query: the tile height for a channel count",
    "drs_conv_workspace_floats": "pure size query",
    "drs_conv_halo_skip": "pure host query of a launch rule: answers 0 for a shape the convolution would reject",
    "drs_conv_wgrad_splits": "pure size query",
    "drs_split_conv_mtile": "pure size query",
    "drs_conv_wgrad_split_splits": "pure size query",
    "drs_colsum_scratch_doubles": "pure size query",
    "drs_bn_backward_rows": "pure size query",
    "drs_se_core_sums_scratch_doubles": "pure size query",
    "drs_classifier_rows": "pure size query",
    "drs_temperature_scratch_doubles": "pure size query",
}
STEP_LEVEL = "the step level (drs_net_*, drs_train_step, ...): tests/test_engine_plan.py covers its argument checks"


# ------------------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, name, args, change=None):
    fn = getattr(lib, name)
    a = dict(args)
    if change:
        assert set(change) <= set(a), (name, change)
        a.update(change)
    vals = [a[k] for k, _ in args]
    if len(vals) == len(fn.argtypes):          # (a host-side call without a stream)
        return fn(*vals)
    assert len(vals) + 1 == len(fn.argtypes), (name, len(vals), len(fn.argtypes))        # + the stream, which every row leaves NULL
    return fn(*vals, None)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_baseline_is_inside_the_domain(lib, name):
    """not DRS_ERR_ARG: validation passed.  What comes back is the launch's status (DRS_ERR_HIP without a device), or DRS_OK from a
    call that has nothing to launch."""
    args, _ = ROWS[name]
    rc = _call(lib, name, args)
    assert rc != ERR_ARG and rc in (OK, ERR_HIP), (name, rc)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_every_violation_is_rejected(lib, name):
    args, bad = ROWS[name]
    assert bad, name
    wrong = [(change, rc) for change in bad for rc in [_call(lib, name, args, change)] if rc != ERR_ARG]
    assert not wrong, "%s: not DRS_ERR_ARG for %r" % (name, wrong)


def test_stitch_strides_at_the_array_limit_are_accepted(lib):
    args, _ = ROWS["drs_stitch_accumulate"]
    for change in STITCH_OK:
        rc = _call(lib, "drs_stitch_accumulate", args, change)
        assert rc != ERR_ARG and rc in (OK, ERR_HIP), (change, rc)


def _declared():
    """names of the `int drs_*(` / `size_t drs_*(` declarations of include/drs.h, split at the step-level banner"""
    text = open(os.path.join(ROOT, "include", "drs.h")).read()
    cut = text.index("Step level: the reference's three `sess.run` call shapes")
    pat = re.compile(r"^(?:int|size_t)\s+(drs_\w+)\s*\(", re.M)
    return pat.findall(text[:cut]), pat.findall(text[cut:])


def test_every_op_level_entry_point_has_a_row_or_a_reason():
    op, step = _declared()
    assert len(op) >= 60 and len(step) >= 30 and "drs_conv_forward" in op and "drs_boundary_histogram" in op and "drs_train_step" in step
    assert len(set(op)) == len(op)
    missing = [n for n in op if n not in ROWS and n not in EXCLUDED]
    assert not missing, "op-level entry points with neither a table row nor an exclusion: %r" % missing
    stale = [n for n in list(ROWS) + list(EXCLUDED) if n not in op]
    assert not stale, "rows or exclusions that include/drs.h does not declare at the op level: %r" % stale
    assert not set(ROWS) & set(EXCLUDED)
    assert all(isinstance(r, str) and r for r in EXCLUDED.values()) and STEP_LEVEL
    assert not set(step) & (set(ROWS) | set(EXCLUDED))
