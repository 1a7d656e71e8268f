"""Command line: the reference's positional surface, unchanged.

isprs flavour  (isprs_dilated_random.py:1987-2042, 16 arguments):
    input_path output_path currentModelPath trainingInstances testing_instances learningRate weight_decay
    batch_size niter reference_crop_size reference_stride_crop net_type distribution_type probValues update_type process
  + optionally, anywhere, `--dense-tile[=T]` (validate_test / generate_final_maps): overlap-tile inference instead of the
    reference's sliding windows (loops.predict_tile_dense; T = tile side, default min(h, w, 512))
  + optionally, anywhere, with --dense-tile only, `--dense-tta=flip|d4`: its dihedral test-time augmentation (the mean of the class
    probabilities over the flipped / rotated tiles; predict_tile_dense's tta)
  + optionally, anywhere, with --dense-tile only, `--dense-scales=0.75,1,1.25`: its multi-scale test-time augmentation (the sum of
    the class probabilities of the image resampled by each factor, resampled back; predict_tile_dense's scales), with or without
    --dense-tta
  + optionally, anywhere, with --dense-tile only, `--dense-se=global` (nets with squeeze-and-excitation blocks, which --dense-tile
    refuses without it): the blocks are gated by the mean over the whole image, computed exactly in tiles (predict_tile_dense's se)
  + optionally, anywhere, `--score-maps=confidence,margin,entropy` (validate_test / generate_final_maps; with or without --dense-tile and
    its companions): per-pixel uint8 score maps beside the labels -- written as `<stem>_<kind>.npy` / `.tif` by generate_final_maps --
    and, in validate_test, a calibration line per map (loops.validate_test's / generate_final_maps' score_maps)
  + optionally, anywhere, with --score-maps only, `--calibrate-temperature` (validate_test): temperature scaling: one
    scalar is fitted on the test maps by a first inference pass (loops.fit_temperature), printed, written to
    `<output_path>temperature_step_<N>.npy` (one float32, beta = 1 / T), and validate_test then reports with it
  + optionally, anywhere, with --score-maps only, `--temperature=auto|<T>` (validate_test / generate_final_maps): the score maps are
    of the probabilities at temperature T > 0; `auto` loads the file --calibrate-temperature wrote for the step being evaluated
  + optionally, anywhere, `--crf[=ITERS]` (validate_test / generate_final_maps; any inference path): every map is the posterior
    refined by a local dense CRF against the image (loops.refine_crf), ITERS mean-field iterations (1..10, default 5);
    `--crf-params=R,step,w_app,theta_xy,theta_rgb,w_smooth,theta_s` sets its window and kernels (default 5,2,4,8,0.08,2,2) and alone
    implies --crf.  With --crf a --temperature is accepted without --score-maps: it scales the unary and can change labels
  + optionally, anywhere, `--boundary-scores[=d0,d1,...]` (validate_test; any inference path, with or without --crf): one more line per
    map and for all maps with the trimap accuracy and the Boundary IoU at the distances given (pixels; 1 to 8 ascending integers in
    1..16; the bare flag means 1,2,4,8) and the plain IoU (loops.validate_test's boundary_scores)
  + optionally, anywhere, `--sieve=N|n0,n1,...,n5` (validate_test / generate_final_maps; any inference path, with or without --crf):
    a minimum mapping unit: every map is sieved before anything scores or writes it -- connected regions of a class k below n_k pixels
    (N: the same threshold for every class; 0: leave the class alone) merge into their largest neighbouring region that is itself large
    enough, round after round until none is left (loops.sieve_labels); one `Sieve` line per map and for all maps.
    `--sieve-connectivity=4|8` (default 4; with --sieve only) says what holds a region together.  Score maps and calibration lines
    stay those of the unsieved labels
  + optionally, anywhere, `--superpixel-vote[=size[,compactness[,iters]]]` (validate_test / generate_final_maps; any inference path,
    after --crf and before --sieve): object-based voting: the map's image is cut into superpixels (integer SLIC; grid step `size`
    4..32, default 8; compactness 1..40, default 10; 1..16 iterations, default 5) and every connected piece of a superpixel takes the
    class most of its pixels voted for, ties to the lower class (loops.superpixel_vote); one `Superpixel` line per
    map and for all maps.  `--superpixel-weight=labels|confidence` (default labels; with --superpixel-vote only): with `confidence`
    a pixel votes with its confidence byte.  Score maps and calibration lines stay those of the unvoted labels
  + optionally, anywhere, `--polygons[=4|8]` (generate_final_maps; any inference path, after --crf, --superpixel-vote and --sieve):
    the map that is written is also written as polygons, `<stem>.geojson` beside `<stem>.tif` / `.npy`: one Polygon feature per
    connected region of a class (4-connected by default; the bare flag takes --sieve-connectivity where --sieve is given), exterior
    ring first, then its holes, on the pixel-corner lattice with collinear points dropped (loops.polygons, vectors.geojson;
    DESIGN.md 8a.12); one `Polygons` line per map and for all maps
  + optionally, anywhere, `--object-scores[=4|8]` (validate_test; any inference path, with or without --crf / --sieve): one more line
    per map and for all maps with object-level scores -- the connected regions of each class (4-connected by default) are the objects,
    a truth object and a predicted one match when their IoU exceeds 1/2 --: per class the truth / predicted / matched counts, detection
    precision, recall and F1, the mean IoU of the matched objects (SQ) and the panoptic quality PQ (loops.validate_test's
    object_scores)
  + optionally, anywhere, `--surface-scores[=t0,t1,...]` (validate_test; any inference path, with or without --crf / --sieve): one
    more line per map and for all maps with surface-distance scores from an exact, unbounded distance transform -- per class the
    average symmetric surface distance, the Hausdorff distance at the 95th percentile and at the maximum, and the normalised surface
    Dice at the tolerances given (pixels; 1 to 8 ascending integers in 1..255; the bare flag means 1,2,4,8) (loops.validate_test's
    surface_scores)
  + optionally, anywhere, in all three flavours, `--class-weights=balanced|median|w0,w1,...` (training): per-class weights of the
    cross-entropy, from the training labels' pixel counts or as given, one per class (loops.train's class_weights)
  + optionally, anywhere, in all three flavours, `--focal-gamma=G` (training; with or without --class-weights): the focusing parameter
    of the focal loss, 0 or in (0, 8] (loops.train's focal_gamma)
  + optionally, anywhere, in all three flavours, `--boundary-weight=a[,sigma[,R]]` (training; on top of --class-weights and
    --focal-gamma): every pixel's loss term is multiplied by 1 + a exp(-d^2 / 2 sigma^2), d the distance to the nearest pixel of
    another class inside the patch and a (2R + 1)^2 window; a in [-1, 64] (0: off), sigma in (0, 64] (default 4), R in 1..16
    (default min(16, ceil(3 sigma))) (loops.train's boundary_weight)
  + optionally, anywhere, in all three flavours, `--dice-weight=lam[,alpha,beta[,smooth]]` (training; beside --class-weights,
    --focal-gamma and --boundary-weight, which do not weight it): lam times a soft Dice / Tversky term per patch is added to the loss;
    lam in [0, 64] (0: off), alpha and beta in [0, 1] (default 0.5,0.5: Dice), smooth in (0, 2^20] (default 1) (loops.train's dice;
    DESIGN.md 3d)
  + optionally, anywhere, in all three flavours, `--lovasz-weight=lam` (training; beside --class-weights, --focal-gamma,
    --boundary-weight and --hard-mining, which do not weight it, and --dice-weight): lam times the Lovasz-softmax loss per patch, over
    the classes present in it, is added to the loss; lam in [0, 64] (0: off) (loops.train's lovasz)
  + optionally, anywhere, in all three flavours, `--surface-loss=lam[,clip]` (training; beside --class-weights, --focal-gamma,
    --boundary-weight and --hard-mining, which do not weight it, --dice-weight and --lovasz-weight): the boundary (surface) loss per
    patch -- the softmax probabilities against lam times the signed Euclidean distance maps of the patch's labels, clipped to +-clip
    pixels when clip > 0 -- is added to the loss; lam in [0, 64] (0: off), clip 0 (none, the default) or in [1, 32768]
    (loops.train's surface_loss)
  + optionally, anywhere, in all three flavours, `--hard-mining=keep[,min_keep]` (training; beside --class-weights, --focal-gamma,
    --boundary-weight, which shape the terms it selects among, and --dice-weight, which it does not touch): online hard example
    mining -- the cross-entropy runs over the max(ceil(keep n), min_keep) of a patch's n in-loss pixels with the largest plain
    cross-entropy; keep in (0, 1] (1: off), min_keep an integer in [0, 2^24) (default 0) (loops.train's hard_mining)
  + optionally, anywhere, in all three flavours, `--scale-jitter=lo,hi` (training): every training patch is resampled at a scale
    drawn log-uniformly from [lo, hi], 0.25 <= lo <= hi <= 4 (loops.train's scale_jitter); validation and inference
    stay at scale 1
coffee / contest flavours (coffee_dilated_random.py:1106-1150, contest_dilated_random.py:1229-1271, 14 [+ operation]):
    path_train path_test output_path currentModelPath lr wd batch niter ref_crop ref_stride net_type distribution_type
    probValues update_type [operation]

Tiles come from the ISPRS Vaihingen / Potsdam directory layouts (datasets.py: Pillow in place of the reference's
gdal / scipy.misc / skimage), from `<input_path><instance>.npz` (arrays `image` [H,W,C] float in [0,1], `label` [H,W]
uint8), or are generated when input_path is `synthetic:<H>x<W>x<C>/<dataset-name>/`.
"""
import os
import sys
import zlib

import numpy as np

from . import loops, patches as P, sampling as SP
from .net import NoComm
from .nets import resolve
from .synthetic import make_tile

ISPRS_PARAMS = ["input_path", "output_path(for model, images, etc)", "currentModelPath", "trainingInstances",
                "testing_instances", "learningRate", "weight_decay", "batch_size", "niter", "reference_crop_size",
                "reference_stride_crop",
                "net_type[dilated_icpr_original|dilated_grsl|dilated_icpr_rate6_densely|dilated_grsl_rate8|dilated8_grsl]",
                "distribution_type[single_fixed|multi_fixed|uniform|multinomial]", "probValues", "update_type [acc|loss]",
                "process [training|validate_test|generate_final_maps]"]


def _take_flag(argv, flag, parse_value, bare=None):
    """The optional `flag=value` -- or the bare `flag`, where `bare` (its value) says that form exists -- anywhere in argv.  Returns
    (argv without the flag, parse_value(the argument as given, the text after `=`)), or (argv unchanged, as a new list, None) without the
    flag.  The flag given twice raises ValueError; a bare flag that has no bare form reaches parse_value with an empty text, to be
    refused in the flag's own words."""
    rest, found, value = [], False, None
    for a in argv:
        if a != flag and not a.startswith(flag + "="):
            rest.append(a)
            continue
        if found:
            raise ValueError(flag + " given more than once")
        found = True
        value = bare if a == flag and bare is not None else parse_value(a, a[len(flag) + 1:])
    return (rest if found else list(argv)), value


def _or_expected(parse, a, v, expected):
    """parse(v), its ValueError reworded as `<argument>: expected <form>`"""
    try:
        return parse(v)
    except ValueError:
        raise ValueError("%s: expected %s" % (a, expected)) from None


def _one_of(choices, flag):
    def parse(v):
        if v not in choices:
            raise ValueError(v)
        return v
    return lambda a, v: _or_expected(parse, a, v, "%s=%s" % (flag, "|".join(choices)))


DENSE_TILE_FLAG = "--dense-tile"


def parse_dense_tile(argv):
    """isprs flavour: the optional `--dense-tile[=T]` (anywhere in argv) that switches validate_test / generate_final_maps to
    overlap-tile inference (loops.predict_tile_dense).  Returns (argv without the flag, T) -- T = 0 for the bare flag (the default
    side), None without it, in which case argv comes back unchanged.  A malformed value, or the flag given twice, raises ValueError."""
    def side(a, v):
        if not (v.isascii() and v.isdigit()) or int(v) < 1:
            raise ValueError("%s=%s: the tile side must be a positive integer" % (DENSE_TILE_FLAG, v))
        return int(v)
    return _take_flag(argv, DENSE_TILE_FLAG, side, bare=0)


DENSE_TTA_FLAG = "--dense-tta"


def parse_dense_tta(argv):
    """isprs flavour: the optional `--dense-tta=flip|d4` (anywhere in argv; with --dense-tile only, which main checks).  Returns (argv
    without the flag, "flip" / "d4"), or (argv unchanged, None) without it.  Any other value, a bare flag, or the flag given twice,
    raises ValueError."""
    return _take_flag(argv, DENSE_TTA_FLAG, _one_of(P.TTA_GROUPS, DENSE_TTA_FLAG))


DENSE_SCALES_FLAG = "--dense-scales"


def parse_dense_scales(argv):
    """isprs flavour: the optional `--dense-scales=s1,s2,...` (anywhere in argv; with --dense-tile only, which main checks).  Returns
    (argv without the flag, tuple of floats; patches.check_scales), or (argv unchanged, None) without it.  A bare flag, a malformed
    or invalid list, or the flag given twice, raises ValueError."""
    def factors(v):
        if not v or v != v.strip() or " " in v:
            raise ValueError(v)
        return [float(t) for t in v.split(",")]
    return _take_flag(argv, DENSE_SCALES_FLAG, lambda a, v: P.check_scales(_or_expected(
        factors, a, v, DENSE_SCALES_FLAG + "=s1,s2,... (factors such as 0.75,1,1.25)")))


DENSE_SE_FLAG = "--dense-se"


def parse_dense_se(argv):
    """isprs flavour: the optional `--dense-se=global` (anywhere in argv; with --dense-tile only, which main checks).  Returns (argv
    without the flag, "global"), or (argv unchanged, None) without it.  Any other value, a bare flag, or the flag given twice, raises
    ValueError."""
    return _take_flag(argv, DENSE_SE_FLAG, _one_of(loops.DENSE_SE_MODES, DENSE_SE_FLAG))


SCORE_MAPS_FLAG = "--score-maps"


def parse_score_maps(argv):
    """isprs flavour: the optional `--score-maps=kind,kind,...` (anywhere in argv; validate_test / generate_final_maps, which main
    checks).  Returns (argv without the flag, tuple of kinds; patches.parse_score_maps), or (argv unchanged, None) without it.  A bare
    flag, an unknown or repeated kind, or the flag given twice, raises ValueError."""
    return _take_flag(argv, SCORE_MAPS_FLAG, lambda a, v: _or_expected(
        P.parse_score_maps, a, v, "%s=%s (distinct kinds from these, comma-separated)" % (SCORE_MAPS_FLAG, ",".join(P.SCORE_KINDS))))


CALIBRATE_FLAG = "--calibrate-temperature"
TEMPERATURE_FLAG = "--temperature"


def parse_calibrate_temperature(argv):
    """isprs flavour: the optional bare `--calibrate-temperature` (anywhere in argv; validate_test with --score-maps, which main
    checks).  Returns (argv without the flag, True), or (argv unchanged, None) without it.  A value, or the flag given twice, raises
    ValueError."""
    def no_value(a, v):
        raise ValueError("%s: %s takes no value" % (a, CALIBRATE_FLAG))
    return _take_flag(argv, CALIBRATE_FLAG, no_value, bare=True)


def parse_temperature(argv):
    """isprs flavour: the optional `--temperature=auto|T` (anywhere in argv; validate_test / generate_final_maps with --score-maps,
    which main checks).  Returns (argv without the flag, "auto" or the inverse temperature beta = 1 / T; patches.parse_temperature), or
    (argv unchanged, None) without it.  A bare flag, a value that is neither, or the flag given twice, raises ValueError."""
    return _take_flag(argv, TEMPERATURE_FLAG, lambda a, v: _or_expected(
        P.parse_temperature, a, v, "%s=auto or %s=T with a temperature T > 0, 1/64 <= 1/T <= 64" % (TEMPERATURE_FLAG, TEMPERATURE_FLAG)))


def temperature_file(output_path, step):
    """where --calibrate-temperature writes, and --temperature=auto reads, the fitted inverse temperature of a step: beside the size
    scores (patch_acc_loss_step_<N>.npy)"""
    return output_path + "temperature_step_" + str(step) + ".npy"


CRF_FLAG = "--crf"
CRF_PARAMS_FLAG = "--crf-params"


def parse_crf(argv):
    """isprs flavour: the optional `--crf[=ITERS]` and `--crf-params=R,step,w_app,theta_xy,theta_rgb,w_smooth,theta_s` (anywhere in
    argv; validate_test / generate_final_maps, which main checks).  Returns (argv without the flags, the patches.CrfParams of
    patches.check_crf), or (argv unchanged, None) without either; --crf-params alone implies --crf.  A malformed or out-of-range
    value, or a flag given twice, raises ValueError."""
    argv, iters = _take_flag(argv, CRF_FLAG, lambda a, v: _or_expected(
        P.parse_crf_iters, a, v, "%s or %s=ITERS (iterations, 1..%d)" % (CRF_FLAG, CRF_FLAG, P.CRF_MAX_ITERS)), bare=P.CRF_DEFAULTS.iters)
    argv, params = _take_flag(argv, CRF_PARAMS_FLAG, lambda a, v: _or_expected(
        P.parse_crf_params, a, v, "%s=%s (%s)" % (CRF_PARAMS_FLAG, ",".join(P.CrfParams._fields[1:]), P.CRF_FORM)))
    if iters is None and params is None:
        return argv, None
    spec = dict(params or {})
    if iters is not None:
        spec["iters"] = iters
    return argv, P.check_crf(spec)


BOUNDARY_FLAG = "--boundary-scores"


def parse_boundary_scores(argv):
    """isprs flavour: the optional `--boundary-scores[=d0,d1,...]` (anywhere in argv; validate_test, which main checks).  Returns (argv
    without the flag, tuple of distances; patches.parse_boundary_scores) -- patches.BOUNDARY_DEFAULT for the bare flag --, or (argv
    unchanged, None) without it.  A malformed or invalid list, or the flag given twice, raises ValueError."""
    return _take_flag(argv, BOUNDARY_FLAG, lambda a, v: _or_expected(
        P.parse_boundary_scores, a, v, "%s or %s=d0,d1,... (1 to %d ascending integers in 1..%d, such as 1,2,4,8)"
        % (BOUNDARY_FLAG, BOUNDARY_FLAG, P.BOUNDARY_MAX_DISTANCES, P.BOUNDARY_MAX_REACH)), bare=P.BOUNDARY_DEFAULT)


SIEVE_FLAG = "--sieve"
SIEVE_CONNECTIVITY_FLAG = "--sieve-connectivity"


def parse_sieve(argv, num_classes=None):
    """isprs flavour: the optional `--sieve=N|n0,n1,...` and `--sieve-connectivity=4|8` (anywhere in argv; validate_test /
    generate_final_maps, which main checks).  Returns (argv without the flags, the patches.SieveParams of patches.check_sieve), or
    (argv unchanged, None) without either.  A bare --sieve, a malformed or out-of-range value, a count of thresholds other than 1 or
    num_classes (when given), --sieve-connectivity without --sieve, or a flag given twice, raises ValueError."""
    form = "%s=N or %s=n0,n1,... (%s integers in 0..2^30, pixels)" % (SIEVE_FLAG, SIEVE_FLAG,
                                                                     "one or one per class:" if num_classes is None else "1 or %d" % num_classes)

    def sizes(a, v):
        ms = _or_expected(P.parse_sieve, a, v, form)
        if num_classes is not None and len(ms) not in (1, num_classes):
            raise ValueError("%s: %d thresholds given, expected %s" % (a, len(ms), form))
        return ms
    argv, min_size = _take_flag(argv, SIEVE_FLAG, sizes)
    argv, conn = _take_flag(argv, SIEVE_CONNECTIVITY_FLAG, _one_of(("4", "8"), SIEVE_CONNECTIVITY_FLAG))
    if min_size is None:
        if conn is not None:
            raise ValueError(SIEVE_CONNECTIVITY_FLAG + " applies to the sieve only: give " + SIEVE_FLAG + " as well")
        return argv, None
    return argv, P.check_sieve(dict(min_size=min_size, connectivity=P.SIEVE_CONNECTIVITY if conn is None else int(conn)))


SUPERPIXEL_FLAG = "--superpixel-vote"
SUPERPIXEL_WEIGHT_FLAG = "--superpixel-weight"


def parse_superpixel(argv):
    """isprs flavour: the optional `--superpixel-vote[=size[,compactness[,iters]]]` and `--superpixel-weight=labels|confidence`
    (anywhere in argv; validate_test / generate_final_maps, which main checks).  Returns (argv without the flags, the
    patches.SuperpixelParams of patches.check_superpixel) -- the defaults for the bare flag --, or (argv unchanged, None) without
    either.  A malformed or out-of-range value, --superpixel-weight without --superpixel-vote, or a flag given twice, raises
    ValueError."""
    ranges = ", ".join("%s %d..%d" % r for r in P.SUPERPIXEL_RANGES)
    argv, values = _take_flag(argv, SUPERPIXEL_FLAG, lambda a, v: _or_expected(
        P.parse_superpixel, a, v, "%s or %s=size[,compactness[,iters]] (integers: %s)" % (SUPERPIXEL_FLAG, SUPERPIXEL_FLAG, ranges)),
        bare=())
    argv, weight = _take_flag(argv, SUPERPIXEL_WEIGHT_FLAG, _one_of(P.SUPERPIXEL_WEIGHTS, SUPERPIXEL_WEIGHT_FLAG))
    if values is None:
        if weight is not None:
            raise ValueError(SUPERPIXEL_WEIGHT_FLAG + " applies to the superpixel vote only: give " + SUPERPIXEL_FLAG + " as well")
        return argv, None
    spec = dict(zip(("size", "compactness", "iters"), values))
    if weight is not None:
        spec["weight"] = weight
    return argv, P.check_superpixel(spec)


POLYGONS_FLAG = "--polygons"


def parse_polygons(argv, sieve=None):
    """isprs flavour: the optional `--polygons[=4|8]` (anywhere in argv; generate_final_maps, which main checks).  Returns (argv
    without the flag, the connectivity; patches.parse_polygons), or (argv unchanged, None) without it.  The bare flag takes the
    connectivity of `sieve` (the SieveParams of parse_sieve) where a sieve is given -- the written polygons are then cut as the sieved
    objects were --, else patches.POLYGON_CONNECTIVITY.  Any other value, or the flag given twice, raises ValueError."""
    argv, conn = _take_flag(argv, POLYGONS_FLAG, lambda a, v: _or_expected(
        P.parse_polygons, a, v, "%s or %s=4|8 (what holds a polygon together)" % (POLYGONS_FLAG, POLYGONS_FLAG)), bare=0)
    if conn == 0:
        conn = P.POLYGON_CONNECTIVITY if sieve is None else sieve.connectivity
    return argv, conn


OBJECT_SCORES_FLAG = "--object-scores"


def parse_object_scores(argv):
    """isprs flavour: the optional `--object-scores[=4|8]` (anywhere in argv; validate_test, which main checks).  Returns (argv without
    the flag, the connectivity; patches.parse_object_scores) -- patches.OBJECT_CONNECTIVITY for the bare flag --, or (argv unchanged,
    None) without it.  Any other value, or the flag given twice, raises ValueError."""
    return _take_flag(argv, OBJECT_SCORES_FLAG, lambda a, v: _or_expected(
        P.parse_object_scores, a, v, "%s or %s=4|8 (what holds an object together)" % (OBJECT_SCORES_FLAG, OBJECT_SCORES_FLAG)),
        bare=P.OBJECT_CONNECTIVITY)


SURFACE_SCORES_FLAG = "--surface-scores"


def parse_surface_scores(argv):
    """isprs flavour: the optional `--surface-scores[=t0,t1,...]` (anywhere in argv; validate_test, which main checks).  Returns (argv
    without the flag, tuple of tolerances; patches.parse_surface_scores) -- patches.SURFACE_DEFAULT for the bare flag --, or (argv
    unchanged, None) without it.  A malformed or invalid list, or the flag given twice, raises ValueError."""
    return _take_flag(argv, SURFACE_SCORES_FLAG, lambda a, v: _or_expected(
        P.parse_surface_scores, a, v, "%s or %s=t0,t1,... (1 to %d ascending integers in 1..%d, such as 1,2,4,8)"
        % (SURFACE_SCORES_FLAG, SURFACE_SCORES_FLAG, P.SURFACE_MAX_TOLERANCES, P.SURFACE_MAX_TOLERANCE)), bare=P.SURFACE_DEFAULT)


CLASS_WEIGHTS_FLAG = "--class-weights"


def parse_class_weights(argv, num_classes=None):
    """all flavours: the optional `--class-weights=balanced|median|w0,w1,...` (anywhere in argv; training).  Returns (argv without the
    flag, "balanced" / "median" / tuple of floats), or (argv unchanged, None) without it.  A bare flag, a malformed list, a negative
    or non-finite weight, a list whose length is not num_classes (when given), or the flag given twice, raises ValueError."""
    form = "%s=%s|w0,w1,... (%s finite weights >= 0)" % (CLASS_WEIGHTS_FLAG, "|".join(P.CLASS_WEIGHT_RECIPES),
                                                         "one per class:" if num_classes is None else str(num_classes))

    def weights(a, v):
        cw = _or_expected(P.parse_class_weights, a, v, form)
        if not isinstance(cw, str) and num_classes is not None and len(cw) != num_classes:
            raise ValueError("%s: %d weights given, expected %s" % (a, len(cw), form))
        return cw
    return _take_flag(argv, CLASS_WEIGHTS_FLAG, weights)


FOCAL_GAMMA_FLAG = "--focal-gamma"


def parse_focal_gamma(argv):
    """all flavours: the optional `--focal-gamma=G` (anywhere in argv; training).  Returns (argv without the flag, G as a float), or
    (argv unchanged, None) without it.  A bare flag, a value that is not one number, 0 or finite in (0, 8], or the flag given twice,
    raises ValueError."""
    return _take_flag(argv, FOCAL_GAMMA_FLAG, lambda a, v: _or_expected(
        P.parse_focal_gamma, a, v, "%s=G (one number, 0 or finite in (0, %g])" % (FOCAL_GAMMA_FLAG, P.MAX_FOCAL_GAMMA)))


BOUNDARY_WEIGHT_FLAG = "--boundary-weight"


def parse_boundary_weight(argv):
    """all flavours: the optional `--boundary-weight=a[,sigma[,R]]` (anywhere in argv; training).  Returns (argv without the flag,
    (a, sigma, R) with the defaults filled in), or (argv unchanged, None) without it.  A bare flag, a value outside the ranges of
    patches.check_boundary_weight, or the flag given twice, raises ValueError."""
    return _take_flag(argv, BOUNDARY_WEIGHT_FLAG, lambda a, v: _or_expected(
        P.parse_boundary_weight, a, v, "%s=a[,sigma[,R]] (a in [-1, %g], sigma in (0, %g], R an integer in 1..%d)" % (
            BOUNDARY_WEIGHT_FLAG, P.MAX_BOUNDARY_A, P.MAX_BOUNDARY_SIGMA, P.MAX_BOUNDARY_R)))


DICE_FLAG = "--dice-weight"


def parse_dice(argv):
    """all flavours: the optional `--dice-weight=lam[,alpha,beta[,smooth]]` (anywhere in argv; training).  Returns (argv without the
    flag, (lam, alpha, beta, smooth) with the defaults filled in), or (argv unchanged, None) without it.  A bare flag, a value outside
    the ranges of patches.check_dice, or the flag given twice, raises ValueError."""
    return _take_flag(argv, DICE_FLAG, lambda a, v: _or_expected(
        P.parse_dice, a, v, "%s=lam[,alpha,beta[,smooth]] (lam in [0, %g], alpha and beta in [0, 1], smooth in (0, %g])" % (
            DICE_FLAG, P.MAX_DICE_LAMBDA, P.MAX_DICE_SMOOTH)))


HARD_MINING_FLAG = "--hard-mining"


def parse_hard_mining(argv):
    """all flavours: the optional `--hard-mining=keep[,min_keep]` (anywhere in argv; training).  Returns (argv without the flag, (keep,
    min_keep) with the default filled in), or (argv unchanged, None) without it.  A bare flag, a value outside the ranges of
    patches.check_hard_mining, or the flag given twice, raises ValueError."""
    return _take_flag(argv, HARD_MINING_FLAG, lambda a, v: _or_expected(
        P.parse_hard_mining, a, v, "%s=keep[,min_keep] (keep in (0, 1], min_keep an integer in [0, %d])" % (
            HARD_MINING_FLAG, P.MAX_HARD_MIN_KEEP)))


LOVASZ_FLAG = "--lovasz-weight"


def parse_lovasz(argv):
    """all flavours: the optional `--lovasz-weight=lam` (anywhere in argv; training).  Returns (argv without the flag, lam), or (argv
    unchanged, None) without it.  A bare flag, a value outside the range of patches.check_lovasz, or the flag given twice, raises
    ValueError."""
    return _take_flag(argv, LOVASZ_FLAG, lambda a, v: _or_expected(
        P.parse_lovasz, a, v, "%s=lam (lam in [0, %g])" % (LOVASZ_FLAG, P.MAX_LOVASZ_LAMBDA)))


SURFACE_LOSS_FLAG = "--surface-loss"


def parse_surface_loss(argv):
    """all flavours: the optional `--surface-loss=lam[,clip]` (anywhere in argv; training).  Returns (argv without the flag, (lam, clip)
    with the default filled in), or (argv unchanged, None) without it.  A bare flag, a value outside the ranges of
    patches.check_surface_loss, or the flag given twice, raises ValueError."""
    return _take_flag(argv, SURFACE_LOSS_FLAG, lambda a, v: _or_expected(
        P.parse_surface_loss, a, v, "%s=lam[,clip] (lam in [0, %g], clip 0 or in [1, %g])" % (
            SURFACE_LOSS_FLAG, P.MAX_SURFACE_LAMBDA, P.MAX_SURFACE_CLIP)))


SCALE_JITTER_FLAG = "--scale-jitter"


def parse_scale_jitter(argv):
    """all flavours: the optional `--scale-jitter=lo,hi` (anywhere in argv; training).  Returns (argv without the flag, (lo, hi) as
    floats), or (argv unchanged, None) without it.  A bare flag, a value that is not two finite numbers lo <= hi inside [0.25, 4], or
    the flag given twice, raises ValueError."""
    return _take_flag(argv, SCALE_JITTER_FLAG, lambda a, v: _or_expected(
        P.parse_scale_jitter, a, v, "%s=lo,hi (two numbers, %g <= lo <= hi <= %g)" % (SCALE_JITTER_FLAG, P.SCALE_MIN, P.SCALE_MAX)))


def print_params(list_params, argv):
    print("+" * 97)
    for i in range(1, len(argv)):
        print(list_params[i - 1] + "= " + argv[i])
    print("+" * 97)


def load_images(path, instances, process, num_classes=6, dataset=None):
    """isprs:187-242.  The ISPRS directory layouts go through datasets.load_images (Pillow instead of
    scipy.misc / gdal); `<instance>.npz` tiles and `synthetic:` paths are this build's additions."""
    from . import datasets
    if not path.startswith("synthetic:") and (os.path.isdir(os.path.join(path, "top")) or os.path.isdir(os.path.join(path, "4_Ortho_RGBIR"))):
        return datasets.load_images(path, instances, process, image_type=dataset)
    images, masks = [], []
    for f in instances:
        print(loops.BatchColors.OKBLUE + "Reading instance " + str(f) + loops.BatchColors.ENDC)
        if path.startswith("synthetic:"):
            h, w, c = [int(v) for v in path[len("synthetic:"):].split("/")[0].split("x")]
            img, lab = make_tile(h, w, c, num_classes, seed=zlib.crc32(str(f).encode()) % (2 ** 31))
        else:
            with np.load(os.path.join(path, str(f) + ".npz")) as d:
                img, lab = np.asarray(d["image"], dtype=np.float64), np.asarray(d["label"], dtype=np.uint8)
        images.append(img)
        masks.append(lab)
    return images, masks


def init_size_scores(distribution_type, values, occur_init=0):
    """isprs:2054-2064 (contest initialises patch_occur with ones, contest:1275)."""
    if distribution_type == "multi_fixed":
        n = len(values)
    elif distribution_type in ("uniform", "multinomial"):
        n = values[-1] - values[0] + 1
    else:
        return None, None, None, None
    probs = P.define_multinomial_probs(values) if distribution_type == "multinomial" else None
    return (np.zeros(n, dtype=np.float32), np.full(n, occur_init, dtype=np.int32), np.zeros(n, dtype=np.int32), probs)


def _placement(device, comm):
    """(device, comm) of this process: what the caller passed, else from the launcher's environment -- under
    `python -m torch.distributed.run --nproc-per-node N <script> ...` one rank per GPU over RCCL (dist.from_env binds the GPU and
    forms the process group before anything else touches it); a plain launch is the reference's single process on cuda:0."""
    if device is not None:
        return device, comm or NoComm()
    from .dist import from_env
    device, comm = from_env()
    return device, comm or NoComm()


def main(argv=None, device=None, comm=None):
    device, comm = _placement(device, comm)
    argv = list(sys.argv if argv is None else argv)
    try:
        argv, dense_tile = parse_dense_tile(argv)
        argv, dense_tta = parse_dense_tta(argv)
        argv, dense_scales = parse_dense_scales(argv)
        argv, dense_se = parse_dense_se(argv)
        argv, score_maps = parse_score_maps(argv)
        argv, calibrate = parse_calibrate_temperature(argv)
        argv, temperature = parse_temperature(argv)
        argv, crf = parse_crf(argv)
        argv, boundary = parse_boundary_scores(argv)
        argv, sieve = parse_sieve(argv, 6)
        argv, superpixel = parse_superpixel(argv)
        argv, polygons = parse_polygons(argv, sieve)
        argv, objects = parse_object_scores(argv)
        argv, surface = parse_surface_scores(argv)
        argv, class_weights = parse_class_weights(argv, 6)
        argv, focal_gamma = parse_focal_gamma(argv)
        argv, boundary_weight = parse_boundary_weight(argv)
        argv, dice = parse_dice(argv)
        argv, hard_mining = parse_hard_mining(argv)
        argv, lovasz = parse_lovasz(argv)
        argv, surface_loss = parse_surface_loss(argv)
        argv, scale_jitter = parse_scale_jitter(argv)
    except ValueError as e:
        sys.exit(str(e))
    if dense_tta is not None and dense_tile is None:
        sys.exit(DENSE_TTA_FLAG + " applies to overlap-tile inference only: give --dense-tile as well")
    if dense_scales is not None and dense_tile is None:
        sys.exit(DENSE_SCALES_FLAG + " applies to overlap-tile inference only: give --dense-tile as well")
    if dense_se is not None and dense_tile is None:
        sys.exit(DENSE_SE_FLAG + " applies to overlap-tile inference only: give --dense-tile as well")
    if calibrate is not None and score_maps is None:
        sys.exit(CALIBRATE_FLAG + " applies to the score maps only: give --score-maps as well")
    if temperature is not None and score_maps is None and crf is None:
        sys.exit(TEMPERATURE_FLAG + " applies to the score maps only: give --score-maps as well")
    if calibrate is not None and temperature is not None:
        sys.exit(CALIBRATE_FLAG + " fits the temperature it reports with: " + TEMPERATURE_FLAG + " cannot be given as well")
    if len(argv) < len(ISPRS_PARAMS) + 1:
        sys.exit("Usage: " + argv[0] + " " + " ".join(ISPRS_PARAMS))
    if dense_tile is not None and argv[16] not in ("validate_test", "generate_final_maps"):
        sys.exit(DENSE_TILE_FLAG + " applies to the validate_test and generate_final_maps processes only")
    if score_maps is not None and argv[16] not in ("validate_test", "generate_final_maps"):
        sys.exit(SCORE_MAPS_FLAG + " applies to the validate_test and generate_final_maps processes only")
    if calibrate is not None and argv[16] != "validate_test":
        sys.exit(CALIBRATE_FLAG + " applies to the validate_test process only")
    if temperature is not None and argv[16] not in ("validate_test", "generate_final_maps"):
        sys.exit(TEMPERATURE_FLAG + " applies to the validate_test and generate_final_maps processes only")
    if crf is not None and argv[16] not in ("validate_test", "generate_final_maps"):
        sys.exit(CRF_FLAG + " applies to the validate_test and generate_final_maps processes only")
    if boundary is not None and argv[16] != "validate_test":
        sys.exit(BOUNDARY_FLAG + " applies to the validate_test process only")
    if sieve is not None and argv[16] not in ("validate_test", "generate_final_maps"):
        sys.exit(SIEVE_FLAG + " applies to the validate_test and generate_final_maps processes only")
    if superpixel is not None and argv[16] not in ("validate_test", "generate_final_maps"):
        sys.exit(SUPERPIXEL_FLAG + " applies to the validate_test and generate_final_maps processes only")
    if polygons is not None and argv[16] != "generate_final_maps":
        sys.exit(POLYGONS_FLAG + " applies to the generate_final_maps process only")
    if objects is not None and argv[16] != "validate_test":
        sys.exit(OBJECT_SCORES_FLAG + " applies to the validate_test process only")
    if surface is not None and argv[16] != "validate_test":
        sys.exit(SURFACE_SCORES_FLAG + " applies to the validate_test process only")
    if class_weights is not None and argv[16] != "training":
        sys.exit(CLASS_WEIGHTS_FLAG + " applies to the training process only")
    if focal_gamma is not None and argv[16] != "training":
        sys.exit(FOCAL_GAMMA_FLAG + " applies to the training process only")
    if boundary_weight is not None and argv[16] != "training":
        sys.exit(BOUNDARY_WEIGHT_FLAG + " applies to the training process only")
    if dice is not None and argv[16] != "training":
        sys.exit(DICE_FLAG + " applies to the training process only")
    if hard_mining is not None and argv[16] != "training":
        sys.exit(HARD_MINING_FLAG + " applies to the training process only")
    if lovasz is not None and argv[16] != "training":
        sys.exit(LOVASZ_FLAG + " applies to the training process only")
    if surface_loss is not None and argv[16] != "training":
        sys.exit(SURFACE_LOSS_FLAG + " applies to the training process only")
    if scale_jitter is not None and argv[16] != "training":
        sys.exit(SCALE_JITTER_FLAG + " applies to the training process only")
    if comm.rank == 0:
        print_params(ISPRS_PARAMS, argv)
    (input_path, output_path, former_model_path, tr, te, lr, wd, bs, niter, ref_crop, ref_stride, net_type,
     distribution_type, prob_values, update_type, process) = argv[1:17]
    dataset = input_path[:-1].split("/")[-1].lower()
    training_instances, testing_instances = tr.split(","), te.split(",")
    lr_initial, weight_decay, batch_size, niter = float(lr), float(wd), int(bs), int(niter)
    reference_crop_size, reference_stride_crop = int(ref_crop), int(ref_stride)
    values = [int(i) for i in prob_values.split(",")]
    resolve(net_type)
    display_step = 50
    if dataset == "vaihingen":
        resample_batch = 20
    elif dataset == "postdam":
        resample_batch = 10
    else:
        print("Error! No dataset identified: ", dataset)
        resample_batch = 20
    patch_acc_loss, patch_occur, patch_chosen_values, probs = init_size_scores(distribution_type, values)

    print(loops.BatchColors.WARNING + "Reading images..." + loops.BatchColors.ENDC)
    training_data, training_labels = load_images(input_path, training_instances, process, dataset=dataset)
    testing_data, testing_labels = load_images(input_path, testing_instances, process, dataset=dataset)
    tag = os.path.join(os.getcwd(), "dataset_" + dataset + "_crop_" + str(reference_crop_size) + "_stride_" + str(reference_stride_crop))
    train_dist = test_dist = None
    if process == "training":
        train_dist = SP.create_distributions_over_classes(training_labels, reference_crop_size, reference_stride_crop)
        test_dist = SP.create_distributions_over_classes(testing_labels, reference_crop_size, reference_stride_crop)
    # the reference's cwd .npy caches (isprs:2087-2115); under data parallelism rank 0 reads / builds / writes them and
    # every rank receives rank 0's arrays (loops.rank0_cached), so no rank reads a half-written file or skips RNG draws
    rot = None
    if train_dist is not None:
        rot = loops.rank0_cached(comm, tag + "_rotation.npy", lambda: SP.create_rotation_distribution(train_dist))

    def mean_std():
        if os.path.isfile(tag + "_mean.npy"):
            return (np.load(tag + "_mean.npy"), np.load(tag + "_std.npy"))
        dist_for_stats = train_dist or SP.create_distributions_over_classes(training_labels, reference_crop_size, reference_stride_crop)
        ms = SP.dynamically_calculate_mean_and_std(training_data, dist_for_stats, crop_size=25)   # isprs:2109-2110
        np.save(tag + "_mean.npy", ms[0])
        np.save(tag + "_std.npy", ms[1])
        return ms
    mean_full, std_full = loops.rank0_call(comm, mean_std, "the mean / std caches " + tag + "_{mean,std}.npy")

    if process == "training":
        return loops.train(training_data, training_labels, train_dist, rot, testing_data, testing_labels, test_dist,
                           testing_instances, lr_initial, batch_size, niter, weight_decay, mean_full, std_full, update_type,
                           distribution_type, values, patch_acc_loss, patch_occur, patch_chosen_values, probs, resample_batch,
                           output_path, display_step, net_type, dataset, former_model_path, device=device, comm=comm,
                           class_weights=class_weights, focal_gamma=focal_gamma, scale_jitter=scale_jitter,
                           boundary_weight=boundary_weight, dice=dice, hard_mining=hard_mining, lovasz=lovasz,
                           surface_loss=surface_loss)
    from .net import DilatedNet
    step = loops.step_from_model_path(former_model_path)
    sized = distribution_type in ("multi_fixed", "uniform", "multinomial")
    if sized:
        patch_acc_loss = np.load(output_path + "patch_acc_loss_step_" + str(step) + ".npy")
        patch_occur = np.load(output_path + "patch_occur_step_" + str(step) + ".npy")
    s_max = max(values)
    net = DilatedNet(net_type, training_data[0].shape[-1], 6, weight_decay, b_max=batch_size, s_max=s_max, device=device, comm=comm)
    loops.load_checkpoint(net, former_model_path)
    if temperature == "auto":
        if not os.path.isfile(temperature_file(output_path, step)):
            sys.exit(TEMPERATURE_FLAG + "=auto: " + temperature_file(output_path, step) + " is missing (written by validate_test with "
                     + CALIBRATE_FLAG + ")")
        try:
            temperature = P.check_temperature_beta(float(np.load(temperature_file(output_path, step)).reshape(-1)[0]))
        except (ValueError, IndexError) as e:
            sys.exit(TEMPERATURE_FLAG + "=auto: " + temperature_file(output_path, step) + ": " + str(e))
    path_kw = dict(dense_tile=dense_tile, dense_tta=dense_tta, dense_scales=dense_scales, dense_se=dense_se)
    crf_kw = {} if crf is None else dict(crf=crf)          # without the flag the loops are called as they always were
    boundary_kw = {} if boundary is None else dict(boundary_scores=boundary)
    sieve_kw = {} if sieve is None else dict(sieve=sieve)
    superpixel_kw = {} if superpixel is None else dict(superpixel=superpixel)
    polygons_kw = {} if polygons is None else dict(polygons=polygons)
    objects_kw = {} if objects is None else dict(object_scores=objects)
    surface_kw = {} if surface is None else dict(surface_scores=surface)
    if process == "validate_test":
        crop = (loops.select_best_patch_size(distribution_type, values, patch_acc_loss, patch_occur, update_type, debug=True)
                if sized else int(values[0]))
        if calibrate:
            fit = loops.fit_temperature(net, testing_data, testing_labels, batch_size, mean_full, std_full, crop, comm, **path_kw)
            temperature = fit["beta"]
            if comm.rank == 0:
                print("---- Iter " + str(step) + " -- Temperature= " + "{:.6f}".format(fit["temperature"]) +
                      " Beta= " + "{:.6f}".format(fit["beta"]) + " NLL before= " + "{:.6f}".format(fit["nll_before"]) +
                      " after= " + "{:.6f}".format(fit["nll_after"]) + " Pixels= " + str(fit["count"]) +
                      " Iterations= " + str(fit["iterations"]))
                np.save(temperature_file(output_path, step), np.array([fit["beta"]], dtype=np.float32))
        return loops.validate_test(net, testing_data, testing_labels, testing_instances, batch_size, mean_full, std_full, crop,
                                   step, output_path, comm, score_maps=score_maps, temperature_beta=temperature, **path_kw, **crf_kw,
                                   **boundary_kw, **sieve_kw, **superpixel_kw, **objects_kw, **surface_kw)
    if process == "generate_final_maps":
        return loops.generate_final_maps(net, testing_data, testing_instances, batch_size, mean_full, std_full, update_type,
                                         distribution_type, values, dataset, output_path, patch_acc_loss, patch_occur, comm,
                                         score_maps=score_maps, temperature_beta=temperature, **path_kw, **crf_kw,
                                         **sieve_kw, **superpixel_kw, **polygons_kw)
    print(loops.BatchColors.FAIL + "Process " + process + "not found!" + loops.BatchColors.ENDC)


COFFEE_PARAMS = ["path_train", "path_test", "output_path(for model, images, etc)", "currentModelPath", "learningRate",
                 "weight_decay", "batch_size", "niter", "reference_crop_size", "reference_stride_crop", "net_type",
                 "distribution_type[single_fixed|multi_fixed|uniform|multinomial]", "probValues", "update_type [acc|loss]"]
CONTEST_PARAMS = ["path", "output_path(for model, images, etc)", "currentModelPath", "learningRate", "weight_decay", "batch_size",
                  "niter", "crop_size", "stride_crop", "net_type", "distribution_type[single_fixed|multi_fixed|uniform|multinomial]",
                  "probValues", "update_type [acc|loss]", "operation [train|test]"]


def _load_stack(path, num_classes, seed0):
    """coffee `load_images_torch` (coffee:116-125) on a directory of Torch-ASCII dumps; `synthetic:<n>x<H>x<W>x<C>/` generates."""
    from . import datasets
    if path.startswith("synthetic:"):
        n, h, w, c = [int(v) for v in path[len("synthetic:"):].split("/")[0].split("x")]
        tl = [make_tile(h, w, c, num_classes, seed=seed0 + i) for i in range(n)]
        return [t[0].astype(np.float32) for t in tl], [t[1] for t in tl]
    imgs, masks = datasets.load_images_torch(path)
    return list(imgs), [np.squeeze(m).astype(np.uint8) for m in masks]


def main_coffee(argv=None, device=None, comm=None):
    """coffee_dilated_random.py:1105-1150: 2 classes, 3 bands, errorAcc_/errorOccur_/chosenValues_ side files."""
    from . import loops_indexed as LI
    device, comm = _placement(device, comm)
    argv = list(sys.argv if argv is None else argv)
    try:
        argv, class_weights = parse_class_weights(argv, 2)
        argv, focal_gamma = parse_focal_gamma(argv)
        argv, boundary_weight = parse_boundary_weight(argv)
        argv, dice = parse_dice(argv)
        argv, hard_mining = parse_hard_mining(argv)
        argv, lovasz = parse_lovasz(argv)
        argv, surface_loss = parse_surface_loss(argv)
        argv, scale_jitter = parse_scale_jitter(argv)
    except ValueError as e:
        sys.exit(str(e))
    if len(argv) < len(COFFEE_PARAMS) + 1:
        sys.exit("Usage: " + argv[0] + " " + " ".join(COFFEE_PARAMS))
    if comm.rank == 0:
        print_params(COFFEE_PARAMS, argv)
    path_train, path_test, output_path, current_model, lr, wd, bs, niter, ref_crop, ref_stride, net_type, dist, pv, update_type = argv[1:15]
    values = [int(i) for i in pv.split(",")]
    resolve(net_type)
    acc, occ, chosen, probs = init_size_scores(dist, values)
    train_x, train_y = _load_stack(path_train, 2, 100)
    test_x, test_y = _load_stack(path_test, 2, 200)
    cd = LI.create_distributions_over_classes(train_y, int(ref_crop), int(ref_stride), 2)
    mean_full, std_full = LI.create_mean_and_std(train_x, int(ref_crop), int(ref_stride))
    return LI.train(train_x, train_y, test_x, test_y, cd, mean_full, std_full, output_path, current_model, float(lr), float(wd),
                    int(bs), int(niter), net_type, dist, update_type, acc, occ, chosen, probs, values, num_classes=2,
                    side_names=("errorAcc_step_", "errorOccur_step_", "chosenValues_step_"), device=device, comm=comm,
                    quantize_f16=True, class_weights=class_weights, focal_gamma=focal_gamma,     # coffee:293: training patches pass through float16
                    scale_jitter=scale_jitter, boundary_weight=boundary_weight, dice=dice, hard_mining=hard_mining, lovasz=lovasz,
                           surface_loss=surface_loss)


def main_contest(argv=None, device=None, comm=None):
    """contest_dilated_random.py:1228-1313: 7 classes + void label 7, 3 bands, operation train | test."""
    from . import datasets, loops_indexed as LI
    device, comm = _placement(device, comm)
    argv = list(sys.argv if argv is None else argv)
    try:
        argv, class_weights = parse_class_weights(argv, 7)
        argv, focal_gamma = parse_focal_gamma(argv)
        argv, boundary_weight = parse_boundary_weight(argv)
        argv, dice = parse_dice(argv)
        argv, hard_mining = parse_hard_mining(argv)
        argv, lovasz = parse_lovasz(argv)
        argv, surface_loss = parse_surface_loss(argv)
        argv, scale_jitter = parse_scale_jitter(argv)
    except ValueError as e:
        sys.exit(str(e))
    if len(argv) < len(CONTEST_PARAMS) + 1:
        sys.exit("Usage: " + argv[0] + " " + " ".join(CONTEST_PARAMS))
    if comm.rank == 0:
        print_params(CONTEST_PARAMS, argv)
    path, output_path, current_model, lr, wd, bs, niter, crop, stride, net_type, dist, pv, update_type, operation = argv[1:15]
    if focal_gamma is not None and operation != "train":
        sys.exit(FOCAL_GAMMA_FLAG + " applies to the train operation only")
    if boundary_weight is not None and operation != "train":
        sys.exit(BOUNDARY_WEIGHT_FLAG + " applies to the train operation only")
    if dice is not None and operation != "train":
        sys.exit(DICE_FLAG + " applies to the train operation only")
    if hard_mining is not None and operation != "train":
        sys.exit(HARD_MINING_FLAG + " applies to the train operation only")
    if lovasz is not None and operation != "train":
        sys.exit(LOVASZ_FLAG + " applies to the train operation only")
    if surface_loss is not None and operation != "train":
        sys.exit(SURFACE_LOSS_FLAG + " applies to the train operation only")
    if scale_jitter is not None and operation != "train":
        sys.exit(SCALE_JITTER_FLAG + " applies to the train operation only")
    values = [int(i) for i in pv.split(",")]
    resolve(net_type)
    acc, occ, chosen, probs = init_size_scores(dist, values, occur_init=1)            # contest:1275
    if path.startswith("synthetic:"):
        h, w, c = [int(v) for v in path[len("synthetic:"):].split("/")[0].split("x")]
        (tx, ty), (ex, ey) = make_tile(h, w, c, 8, seed=11), make_tile(h, w, c, 8, seed=12)   # label 7 plays the void role
        train_x, train_y, test_x, test_y = [tx.astype(np.float32)], [ty], [ex.astype(np.float32)], [ey]
    else:
        train_x = [datasets.read_torch_ascii(path + "TelopsDatasetCityVisible_20cm_Subset.txt")]
        test_x = [datasets.read_torch_ascii(path + "TelopsDatasetCityVisible.txt")]
        train_y, test_y = [datasets.read_pgm(path + "gt8.pgm").astype(np.uint8)], [datasets.read_pgm(path + "gt_ult8.pgm").astype(np.uint8)]
    cd = LI.create_distributions_over_classes_contest(train_y[0], int(crop), int(stride), 7)       # contest:172-190
    mean_full, std_full = LI.create_mean_and_std_contest(train_x[0], cd, int(crop))                # contest:99-113
    if operation == "train":
        return LI.train(train_x, train_y, test_x, test_y, cd, mean_full, std_full, output_path, current_model, float(lr), float(wd),
                        int(bs), int(niter), net_type, dist, update_type, acc, occ, chosen, probs, values, num_classes=7,
                        void_label=7, device=device, comm=comm, flavour="contest", class_weights=class_weights,
                        focal_gamma=focal_gamma, scale_jitter=scale_jitter, boundary_weight=boundary_weight, dice=dice, hard_mining=hard_mining, lovasz=lovasz,
                           surface_loss=surface_loss)
    if class_weights is not None:
        sys.exit(CLASS_WEIGHTS_FLAG + " applies to the train operation only")
    if operation == "test":
        from .net import DilatedNet
        step = loops.step_from_model_path(current_model)
        sized = dist in ("multi_fixed", "uniform", "multinomial")
        if sized:
            acc = np.load(output_path + "patch_acc_loss_step_" + str(step) + ".npy")
            occ = np.load(output_path + "patch_occur_step_" + str(step) + ".npy")
        net = DilatedNet(net_type, train_x[0].shape[-1], 7, float(wd), b_max=int(bs), s_max=max(values), device=device, comm=comm)
        loops.load_checkpoint(net, current_model)
        cs = loops.select_best_patch_size(dist, values, acc, occ, update_type, debug=True) if sized else int(values[0])
        return loops.validate_test(net, test_x, test_y, ["test"], int(bs), mean_full, std_full, cs, step, output_path, comm, ignore_label=7,
                                   flavour="contest")
    print(loops.BatchColors.FAIL + "Process " + operation + "not found!" + loops.BatchColors.ENDC)


if __name__ == "__main__":
    main()
