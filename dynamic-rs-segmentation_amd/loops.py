"""Step loops: training, patch validation, whole-tile sliding-window inference (and, opt-in, overlap-tile inference).

Host mirror of /root/reference/isprs_dilated_random.py `train` :1621-1851, `validation` :1569-1618,
`validate_test` :1241-1344 and `generate_final_maps` :1854-1957 (control flow, constants, log line formats and
side files), with every per-pixel operation on the device.  Differences that are deliberate:

  * the reference reads `loss`, `pred_up` back every step and runs a per-pixel Python loop on them
    (calc_accuracy_by_crop, isprs:1754); here the confusion matrix and the loss stay on the device and are read back
    ONE STEP LATE (while the next step runs), so the host never stalls the GPU.  The size-score update is a sum, so
    the lag does not change any result; it is flushed before every display / save / validation point;
  * the TensorFlow checkpoint becomes `model-<step>.npz` (same names, same `-<step>` resume convention, isprs:1708-1715);
  * under data parallelism every rank runs the same host code with the same RNG streams and takes its slice of the batch.
"""
import collections
import contextlib
import ctypes
import datetime
import math
import os
import random

import numpy as np
import torch

from . import metrics as MT
from . import patches as P
from . import sampling as SP
from .dist import shard_slice
from .net import DilatedNet, NoComm

EPOCH_NUMBER = 1000      # isprs:1642
VAL_INTERVAL = 1000      # isprs:1643
SUPER_BATCH = 100        # isprs:1632


class BatchColors:
    OKBLUE, OKGREEN, WARNING, FAIL, ENDC = "\033[94m", "\033[92m", "\033[93m", "\033[91m", "\033[0m"


def select_best_patch_size(distribution_type, values, patch_acc_loss, patch_occur, is_loss_or_acc="acc",
                           patch_chosen_values=None, debug=False):
    """isprs:549-608 (mutates patch_occur: zeros -> 1, exactly like the reference)."""
    patch_occur[np.where(patch_occur == 0)] = 1
    patch_mean = patch_acc_loss / patch_occur
    if is_loss_or_acc == "acc":
        i = int(np.argmax(patch_mean))
    elif is_loss_or_acc == "loss":
        order = np.argsort(patch_mean)
        i = int([j for j in order if patch_occur[j] > 0][0])
    else:
        raise ValueError("update_type must be acc or loss")
    if patch_chosen_values is not None:
        patch_chosen_values[i] += 1
    cur = int(values[i]) if distribution_type == "multi_fixed" else values[0] + i
    if debug:
        print("patch_acc_loss", patch_acc_loss)
        print("patch_occur", patch_occur)
        print("patch_mean", patch_mean)
        print("Current patch size ", cur)
        if patch_chosen_values is not None:
            print("Distr of chosen sizes ", patch_chosen_values)
    return cur


def _cm_str(cm):
    return np.array_str(np.asarray(cm)).replace("\n", "")


CLASS_WEIGHTS_SIDE = "class_weights_step_"


def _weights_str(w):
    return str(["{:.6g}".format(float(v)) for v in w])


def save_class_weights(net, output_path, step):
    """the class weights of the training loss, when set, as the side file `class_weights_step_<step>.npy` beside the size scores (they
    are state of the run, not of the model: the .npz keeps the TensorFlow variable set)"""
    w = getattr(net, "class_weights", None)
    if w is not None:
        np.save(output_path + CLASS_WEIGHTS_SIDE + str(step) + ".npy", np.asarray(w, dtype=np.float32))


def load_class_weights(net, former_model_path):
    """set the weights that save_class_weights left beside `<dir>/model-<step>[.npz]`, if any: a resumed run trains the same loss"""
    head, sep, _ = former_model_path.rpartition("model-")
    if not sep:
        return
    path = head + CLASS_WEIGHTS_SIDE + str(step_from_model_path(former_model_path)) + ".npy"
    if os.path.isfile(path):
        net.set_class_weights(np.load(path))
        if getattr(getattr(net, "comm", None), "rank", 0) == 0:
            print("Class weights (restored from " + path + "): weights " + _weights_str(net.class_weights))


FOCAL_GAMMA_SIDE = "focal_gamma_step_"


def save_focal_gamma(net, output_path, step):
    """the focusing parameter of the training loss, when set (> 0), as the side file `focal_gamma_step_<step>.npy` beside the size
    scores: one float32 (state of the run, not of the model, as the class weights are)"""
    g = float(getattr(net, "focal_gamma", 0.0) or 0.0)
    if g > 0.0:
        np.save(output_path + FOCAL_GAMMA_SIDE + str(step) + ".npy", np.asarray(g, dtype=np.float32))


def load_focal_gamma(net, former_model_path):
    """set the gamma that save_focal_gamma left beside `<dir>/model-<step>[.npz]`, if any: a resumed run trains the same loss"""
    head, sep, _ = former_model_path.rpartition("model-")
    if not sep:
        return
    path = head + FOCAL_GAMMA_SIDE + str(step_from_model_path(former_model_path)) + ".npy"
    if os.path.isfile(path):
        net.set_focal_gamma(float(np.load(path)))
        if getattr(getattr(net, "comm", None), "rank", 0) == 0:
            print("Focal loss (restored from " + path + "): gamma " + "{:.6g}".format(net.focal_gamma))


BOUNDARY_WEIGHT_SIDE = "boundary_weight_step_"


def _boundary_weight_str(bw):
    return "a " + "{:.6g}".format(bw[0]) + " sigma " + "{:.6g}".format(bw[1]) + " R " + str(int(bw[2]))


def save_boundary_weight(net, output_path, step):
    """the boundary weight of the training loss, when on, as the side file `boundary_weight_step_<step>.npy` beside the size scores:
    three float64 (a, sigma, R) (state of the run, not of the model, as the class weights and the focal gamma are)"""
    bw = getattr(net, "boundary_weight", None)
    if bw is not None:
        np.save(output_path + BOUNDARY_WEIGHT_SIDE + str(step) + ".npy", np.asarray([bw[0], bw[1], bw[2]], dtype=np.float64))


def load_boundary_weight(net, former_model_path):
    """set the triple that save_boundary_weight left beside `<dir>/model-<step>[.npz]`, if any: a resumed run trains the same loss"""
    head, sep, _ = former_model_path.rpartition("model-")
    if not sep:
        return
    path = head + BOUNDARY_WEIGHT_SIDE + str(step_from_model_path(former_model_path)) + ".npy"
    if os.path.isfile(path):
        a, sigma, radius = np.load(path).tolist()
        net.set_boundary_weight((a, sigma, int(radius)))
        if getattr(getattr(net, "comm", None), "rank", 0) == 0:
            print("Boundary weight (restored from " + path + "): " + _boundary_weight_str(net.boundary_weight))


DICE_SIDE = "dice_step_"


def _dice_str(d):
    return "lambda " + "{:.6g}".format(d[0]) + " alpha " + "{:.6g}".format(d[1]) + " beta " + "{:.6g}".format(d[2]) + " smooth " + "{:.6g}".format(d[3])


def save_dice(net, output_path, step):
    """the soft Dice / Tversky term of the training loss, when on, as the side file `dice_step_<step>.npy` beside the size scores: four
    float64 (lam, alpha, beta, smooth) (state of the run, not of the model, as the other options of the loss are)"""
    d = getattr(net, "dice", None)
    if d is not None:
        np.save(output_path + DICE_SIDE + str(step) + ".npy", np.asarray(d, dtype=np.float64))


def load_dice(net, former_model_path):
    """set the quadruple that save_dice left beside `<dir>/model-<step>[.npz]`, if any: a resumed run trains the same loss"""
    head, sep, _ = former_model_path.rpartition("model-")
    if not sep or not hasattr(net, "set_dice"):
        return
    path = head + DICE_SIDE + str(step_from_model_path(former_model_path)) + ".npy"
    if os.path.isfile(path):
        net.set_dice(tuple(np.load(path).tolist()))
        if getattr(getattr(net, "comm", None), "rank", 0) == 0:
            print("Dice term (restored from " + path + "): " + _dice_str(net.dice))


HARD_MINING_SIDE = "hard_mining_step_"


def _hard_mining_str(h):
    return "keep " + "{:.6g}".format(h[0]) + " min_keep " + str(int(h[1]))


def save_hard_mining(net, output_path, step):
    """hard example mining in the training loss, when on, as the side file `hard_mining_step_<step>.npy` beside the size scores: two
    float64 (keep, min_keep) (state of the run, not of the model, as the other options of the loss are)"""
    h = getattr(net, "hard_mining", None)
    if h is not None:
        np.save(output_path + HARD_MINING_SIDE + str(step) + ".npy", np.asarray(h, dtype=np.float64))


def load_hard_mining(net, former_model_path):
    """set the pair that save_hard_mining left beside `<dir>/model-<step>[.npz]`, if any: a resumed run trains the same loss"""
    head, sep, _ = former_model_path.rpartition("model-")
    if not sep or not hasattr(net, "set_hard_mining"):
        return
    path = head + HARD_MINING_SIDE + str(step_from_model_path(former_model_path)) + ".npy"
    if os.path.isfile(path):
        keep, min_keep = np.load(path).tolist()
        net.set_hard_mining((keep, int(min_keep)))
        if getattr(getattr(net, "comm", None), "rank", 0) == 0:
            print("Hard mining (restored from " + path + "): " + _hard_mining_str(net.hard_mining))


LOVASZ_SIDE = "lovasz_step_"


def _lovasz_str(lam):
    return "lambda " + "{:.6g}".format(lam)


def save_lovasz(net, output_path, step):
    """the Lovasz-softmax term of the training loss, when on, as the side file `lovasz_step_<step>.npy` beside the size scores: one
    float64 (lam) (state of the run, not of the model, as the other options of the loss are)"""
    lam = getattr(net, "lovasz", None)
    if lam is not None:
        np.save(output_path + LOVASZ_SIDE + str(step) + ".npy", np.asarray([lam], dtype=np.float64))


def load_lovasz(net, former_model_path):
    """set lam that save_lovasz left beside `<dir>/model-<step>[.npz]`, if any: a resumed run trains the same loss"""
    head, sep, _ = former_model_path.rpartition("model-")
    if not sep or not hasattr(net, "set_lovasz"):
        return
    path = head + LOVASZ_SIDE + str(step_from_model_path(former_model_path)) + ".npy"
    if os.path.isfile(path):
        net.set_lovasz(float(np.load(path).reshape(-1)[0]))
        if getattr(getattr(net, "comm", None), "rank", 0) == 0:
            print("Lovasz term (restored from " + path + "): " + _lovasz_str(net.lovasz))


SURFACE_LOSS_SIDE = "surface_loss_step_"


def _surface_loss_str(s):
    return "lambda " + "{:.6g}".format(s[0]) + " clip " + ("{:.6g}".format(s[1]) if s[1] else "none")


def save_surface_loss(net, output_path, step):
    """the boundary (surface) loss of the training loss, when on, as the side file `surface_loss_step_<step>.npy` beside the size
    scores: two float64 (lam, clip) (state of the run, not of the model, as the other options of the loss are)"""
    s = getattr(net, "surface_loss", None)
    if s is not None:
        np.save(output_path + SURFACE_LOSS_SIDE + str(step) + ".npy", np.asarray(s, dtype=np.float64))


def load_surface_loss(net, former_model_path):
    """set the pair that save_surface_loss left beside `<dir>/model-<step>[.npz]`, if any: a resumed run trains the same loss"""
    head, sep, _ = former_model_path.rpartition("model-")
    if not sep or not hasattr(net, "set_surface_loss"):
        return
    path = head + SURFACE_LOSS_SIDE + str(step_from_model_path(former_model_path)) + ".npy"
    if os.path.isfile(path):
        lam, clip = np.load(path).tolist()
        net.set_surface_loss((lam, clip))
        if getattr(getattr(net, "comm", None), "rank", 0) == 0:
            print("Surface loss (restored from " + path + "): " + _surface_loss_str(net.surface_loss))


def save_checkpoint(net, output_path, step, patch_acc_loss=None, patch_occur=None, patch_chosen_values=None):
    """saver.save(sess, output_path + 'model', global_step=step) + the three .npy side files (isprs:1798-1802) + the class weights,
    the focal gamma, the boundary weight, the Dice term, the hard mining, the Lovasz term and the surface loss of the loss when set
    (save_class_weights, save_focal_gamma, save_boundary_weight, save_dice, save_hard_mining, save_lovasz, save_surface_loss)."""
    np.savez(output_path + "model-" + str(step) + ".npz", **net.state_dict())
    save_class_weights(net, output_path, step)
    save_focal_gamma(net, output_path, step)
    save_boundary_weight(net, output_path, step)
    save_dice(net, output_path, step)
    save_hard_mining(net, output_path, step)
    save_lovasz(net, output_path, step)
    save_surface_loss(net, output_path, step)
    if patch_acc_loss is not None:
        np.save(output_path + "patch_acc_loss_step_" + str(step) + ".npy", patch_acc_loss)
        np.save(output_path + "patch_occur_step_" + str(step) + ".npy", patch_occur)
        np.save(output_path + "patch_chosen_values_step_" + str(step) + ".npy", patch_chosen_values)


def load_checkpoint(net, former_model_path):
    """`saver_restore.restore(sess, former_model_path)` (isprs:1715): a TensorFlow V2 checkpoint written by the reference
    (`<path>.index` + `.data-*`, read by tf_checkpoint.py) or this build's own `<path>.npz`."""
    import os
    if os.path.isfile(former_model_path + ".index"):
        from . import tf_checkpoint
        tf_checkpoint.load_tf_checkpoint(net, former_model_path)
        print(BatchColors.OKBLUE + "Model restored from " + former_model_path + " (TensorFlow bundle)" + BatchColors.ENDC)
        return
    path = former_model_path if former_model_path.endswith(".npz") else former_model_path + ".npz"
    with np.load(path) as d:
        net.load_state_dict({k: d[k] for k in d.files})
    load_class_weights(net, former_model_path)
    load_focal_gamma(net, former_model_path)
    load_boundary_weight(net, former_model_path)
    load_dice(net, former_model_path)
    load_hard_mining(net, former_model_path)
    load_lovasz(net, former_model_path)
    load_surface_loss(net, former_model_path)
    print(BatchColors.OKBLUE + "Model restored from " + former_model_path + BatchColors.ENDC)


def step_from_model_path(former_model_path):
    """isprs:1709: int(former_model_path.split('-')[-1])."""
    return int(former_model_path.replace(".npz", "").split("-")[-1])


# ------------------------------------------------------------------------------------------------- validation
def validation(net, test_pool, selected_testing_instances, mean_full, std_full, batch_size, step, crop_size, comm=None):
    """isprs:1569-1618: forward-only over the held-out instances at `crop_size`, one confusion matrix.
    Returns (confusion matrix, pixels processed)."""
    comm = comm or NoComm()
    K = net.plan.K
    n = len(selected_testing_instances)
    nb = -(-n // batch_size)
    net.conf.zero_()
    for i in range(nb):
        if i % comm.world != comm.rank:          # batches are independent: round-robin over ranks
            continue
        rows = selected_testing_instances[i * batch_size:min((i + 1) * batch_size, n)]
        for j in range(0, len(rows), net.b_max):
            part = rows[j:j + net.b_max]
            P.crop_to_net(net, test_pool, part, crop_size, mean_full, std_full)
            net.forward(len(part), crop_size, want_logits=False, labels=True)
    cm_dev = net.conf.clone()
    comm.all_reduce_sum(cm_dev)
    cm = cm_dev.cpu().numpy().reshape(K, K).astype(np.uint32)
    total, oa, na = MT.overall_and_normalized(cm)
    if comm.rank == 0:
        print("---- Iter " + str(step) +
              " -- Time " + str(datetime.datetime.now().time()) +
              " -- Validation: Overall Accuracy= " + str(total) +
              " Overall Accuracy= " + "{:.6f}".format(oa) +
              " Normalized Accuracy= " + "{:.6f}".format(na) +
              " F1 Score= " + "{:.4f}".format(MT.f1_macro(cm)) +
              " Kappa= " + "{:.4f}".format(MT.cohen_kappa(cm)) +
              " Confusion Matrix= " + _cm_str(cm))
    return cm, n * crop_size * crop_size


def check_training_labels(pool, num_classes, void_label=None):
    """tf.nn.sparse_softmax_cross_entropy_with_logits raises on a label outside [0, K) (isprs:1093); a label map that holds one
    (an unknown colour from datasets.convert_to_class becomes 255 in the uint8 pool) must not silently enter the loss."""
    bad = pool.labels >= num_classes
    if void_label is not None:
        bad &= pool.labels != void_label
    if bool(bad.any()):
        raise ValueError("training labels hold class ids outside [0, %d): %s" % (num_classes, torch.unique(pool.labels[bad]).tolist()[:8]))


def setup_class_weights(net, pool, num_classes, class_weights, comm, say, void_label=None):
    """The class weights of a training run (train's `class_weights`): "balanced" / "median" from the per-class pixel counts of the
    pool's label maps, counted on the device (TilePool.label_counts; the void label left out), or K numbers as given
    (patches.class_weights).  Every rank holds the same pool and so computes the same weights: asserted once over the ranks, bit
    patterns and counts.  One log line says what is in use."""
    counts = pool.label_counts(num_classes, void_label)
    wc = P.check_class_weights(list(P.class_weights(counts, class_weights)), num_classes)
    comm.agree([int(c) for c in counts] + [int(b) for b in wc.view(np.uint32)], "class counts / class weights")
    restored = net.class_weights
    net.set_class_weights(wc)
    say("Class weights (" + (class_weights if isinstance(class_weights, str) else "given") + "): pixel counts " + str([int(c) for c in counts]) +
        " weights " + _weights_str(wc) +
        ("" if restored is None or restored.tobytes() == wc.tobytes() else " -- replacing the weights restored from the checkpoint, " + _weights_str(restored)))
    return wc


def setup_focal_gamma(net, focal_gamma, comm, say):
    """The focusing parameter of a training run (train's `focal_gamma`; patches.check_focal_gamma): every rank must hold the same one,
    asserted once over the ranks on its float32 bits.  Given, it replaces a gamma restored from a checkpoint's side file.  One log
    line names it; gamma = 0 on a run that restored none is today's run and says nothing."""
    g = P.check_focal_gamma(focal_gamma)
    comm.agree([int(np.asarray(g, dtype=np.float32).view(np.uint32))], "focal gamma")
    restored = float(net.focal_gamma)
    net.set_focal_gamma(g)
    if g > 0.0 or restored != g:
        say("Focal loss: gamma " + "{:.6g}".format(g) + (" (the loss is wc[y] (1 - p_t)^gamma CE)" if g > 0.0 else " (off: the cross-entropy)") +
            ("" if restored == 0.0 or restored == g else " -- replacing the gamma restored from the checkpoint, " + "{:.6g}".format(restored)))
    return g


def setup_boundary_weight(net, boundary_weight, comm, say):
    """The boundary weight of a training run (train's `boundary_weight`; patches.check_boundary_weight): every rank must hold the same
    triple (a, sigma, R), asserted once over the ranks on the float64 bits.  Given, it replaces a triple restored from a checkpoint's
    side file.  One log line names it; a = 0 on a run that restored none is today's run and says nothing."""
    bw = P.check_boundary_weight(boundary_weight)
    bits = np.asarray(bw[:2], dtype=np.float64).view(np.uint32)
    comm.agree([int(b) for b in bits] + [int(bw[2])], "boundary weight")
    restored = net.boundary_weight
    net.set_boundary_weight(bw)
    on = bw[0] != 0.0
    if on or restored is not None:
        say("Boundary weight: " + (_boundary_weight_str(bw) + " (the loss is (1 + a exp(-D2 / 2 sigma^2)) wc[y] m CE, normalised as before)"
                                   if on else "a 0 (off: every pixel weighs one)") +
            ("" if restored is None or restored == bw else " -- replacing the triple restored from the checkpoint, " + _boundary_weight_str(restored)))
    return bw


def setup_dice(net, dice, comm, say):
    """The soft Dice / Tversky term of a training run (train's `dice`; patches.check_dice): every rank must hold the same quadruple
    (lam, alpha, beta, smooth), asserted once over the ranks on the float64 bits.  Given, it replaces a quadruple restored from a
    checkpoint's side file.  One log line names it; lam = 0 on a run that restored none is today's run and says nothing."""
    d = P.check_dice(dice)
    comm.agree([int(b) for b in np.asarray(d, dtype=np.float64).view(np.uint32)], "dice term")
    restored = net.dice
    net.set_dice(d)
    on = d[0] != 0.0
    if on or restored is not None:
        say("Dice term: " + (_dice_str(d) + " (the loss is the cross-entropy part + lambda times the pixel-weighted mean over patches and "
                                            "classes of 1 - Tversky index; class, focal and boundary weights do not weight it)"
                             if on else "lambda 0 (off: the cross-entropy part alone)") +
            ("" if restored is None or restored == d else " -- replacing the quadruple restored from the checkpoint, " + _dice_str(restored)))
    return d


def setup_hard_mining(net, hard_mining, comm, say):
    """Hard example mining of a training run (train's `hard_mining`; patches.check_hard_mining): every rank must hold the same pair
    (keep, min_keep), asserted once over the ranks on the float64 bits of keep and on min_keep.  Given, it replaces a pair restored
    from a checkpoint's side file.  One log line names it; keep = 1 on a run that restored none is today's run and says nothing."""
    h = P.check_hard_mining(hard_mining)
    comm.agree([int(b) for b in np.asarray([h[0]], dtype=np.float64).view(np.uint32)] + [h[1]], "hard mining")
    restored = net.hard_mining
    net.set_hard_mining(h)
    on = h[0] != 1.0
    if on or restored is not None:
        say("Hard mining: " + (_hard_mining_str(h) + " (the cross-entropy part of the loss runs over the max(ceil(keep n), min_keep) of a patch's n "
                                                    "in-loss pixels with the largest plain cross-entropy, each at the weight n / kept; the printed loss is the mined one)"
                               if on else "keep 1 (off: every pixel in the loss)") +
            ("" if restored is None or restored == h else " -- replacing the pair restored from the checkpoint, " + _hard_mining_str(restored)))
    return h


def setup_lovasz(net, lovasz, comm, say):
    """The Lovasz-softmax term of a training run (train's `lovasz`; patches.check_lovasz): every rank must hold the same lam, asserted
    once over the ranks on its float64 bits.  Given, it replaces a value restored from a checkpoint's side file.  One log line names
    it; lam = 0 on a run that restored none is today's run and says nothing."""
    lam = P.check_lovasz(lovasz)
    comm.agree([int(b) for b in np.asarray([lam], dtype=np.float64).view(np.uint32)], "lovasz term")
    restored = net.lovasz
    net.set_lovasz(lam)
    on = lam != 0.0
    if on or restored is not None:
        say("Lovasz term: " + (_lovasz_str(lam) + " (the loss is the cross-entropy part + lambda times the pixel-weighted mean over patches of the "
                                                  "Lovasz-softmax loss over the classes present in the patch; class, focal, boundary and mining weights do not weight it)"
                               if on else "lambda 0 (off: the cross-entropy part alone)") +
            ("" if restored is None or restored == lam else " -- replacing the value restored from the checkpoint, " + _lovasz_str(restored)))
    return lam


def setup_surface_loss(net, surface_loss, comm, say):
    """The boundary (surface) loss of a training run (train's `surface_loss`; patches.check_surface_loss): every rank must hold the
    same pair (lam, clip), asserted once over the ranks on their float64 bits.  Given, it replaces a pair restored from a checkpoint's
    side file.  One log line names it; lam = 0 on a run that restored none is today's run and says nothing."""
    s = P.check_surface_loss(surface_loss)
    comm.agree([int(b) for b in np.asarray(s, dtype=np.float64).view(np.uint32)], "surface loss")
    restored = net.surface_loss
    net.set_surface_loss(s)
    on = s[0] != 0.0
    if on or restored is not None:
        say("Surface loss: " + (_surface_loss_str(s) + " (the loss is the cross-entropy part + lambda times the mean over the pixels in the loss of the "
                                                       "sum over classes of the softmax probability times the class's signed distance map of the patch's "
                                                       "labels; class, focal, boundary and mining weights do not weight it)"
                                if on else "lambda 0 (off: the cross-entropy part alone)") +
            ("" if restored is None or restored == s else " -- replacing the pair restored from the checkpoint, " + _surface_loss_str(restored)))
    return s


def surface_loss_grad(logits, labels, lam, clip=0, loss_mask=None, valid=None, dice_coef=None):
    """The per-(pixel, class) map drs_train_step makes of a step's labels and logits when the boundary (surface) loss is on (DESIGN.md
    3g), for inspection: logits float32 [B, S, S, K] and labels uint8 [B, S, S] (tensors on the GPU, or anything np.asarray takes --
    then on the current device), loss_mask and valid uint8 [B, S, S] or None, dice_coef float32 [B, K, 2] (drs_patch_dice_coeffs'
    output, folded into the map) or None.  Returns (map float32 [B, S, S, K]: g_c(p), 0 where a pixel is not counted; phi2 int64
    [B, S, S, K]: +D2 outside the class, -D2 inside, 0 where the class has no distance map in the patch or the pixel is not counted;
    patch_loss float64 [B]) as tensors on that device.  One call of drs_patch_surface_loss."""
    import torch
    from . import _lib

    def dev(x, dtype):
        if x is None:
            return None
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x))).cuda()
        return x.to(dtype).contiguous()
    lg, lab = dev(logits, torch.float32), dev(labels, torch.uint8)
    if lg.dim() != 4 or lab.dim() != 3 or lg.shape[:3] != lab.shape or lab.shape[1] != lab.shape[2]:
        raise ValueError("surface_loss_grad: logits [B, S, S, K] and labels [B, S, S] expected, got %r and %r" % (tuple(lg.shape), tuple(lab.shape)))
    B, S, K = int(lab.shape[0]), int(lab.shape[1]), int(lg.shape[3])
    lam, clip = P.check_surface_loss((lam, clip))
    lm, va, dc = dev(loss_mask, torch.uint8), dev(valid, torch.uint8), dev(dice_coef, torch.float32)
    if (lm is not None and lm.shape != lab.shape) or (va is not None and va.shape != lab.shape):
        raise ValueError("surface_loss_grad: loss_mask and valid must have the shape of labels")
    if dc is not None and tuple(dc.shape) != (B, K, 2):
        raise ValueError("surface_loss_grad: dice_coef must be [B, K, 2]")
    grad = torch.empty_like(lg)
    phi2 = torch.empty(lg.shape, dtype=torch.int32, device=lab.device)
    loss = torch.empty(B, dtype=torch.float64, device=lab.device)
    nbytes = _lib.query("drs_surface_loss_scratch_bytes", B, S, K)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("drs_patch_surface_loss", lg.data_ptr(), lab.data_ptr(), None if lm is None else lm.data_ptr(),
                  None if va is None else va.data_ptr(), B, S, K, lam, clip, None if dc is None else dc.data_ptr(), 0, phi2.data_ptr(),
                  grad.data_ptr(), loss.data_ptr(), scratch.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    return grad, phi2.to(torch.int64), loss


def lovasz_grad(logits, labels, lam, loss_mask=None, dice_coef=None):
    """The per-(pixel, class) map drs_train_step makes of a step's logits when the Lovasz-softmax term is on, for
    inspection: logits float32 [B, S, S, K] and labels uint8 [B, S, S] (tensors on the GPU, or anything np.asarray takes -- then on
    the current device), loss_mask uint8 [B, S, S] or None, dice_coef float32 [B, K, 2] (drs_patch_dice_coeffs' output, folded into the
    map) or None.  Returns (grad float32 [B, S, S, K]: g_c(p), 0 where a pixel is not in the loss; rank int64 [B, S, S, K]: the 0-based
    position of the pixel in the class's order, -1 where the pixel is not in the loss or the class is absent from the patch; err
    float32 [B, S, S, K]: the error keys; patch_loss float64 [B]) as tensors on that device.  One call of drs_patch_lovasz_grad."""
    import torch
    from . import _lib

    def dev(x, dtype):
        if x is None:
            return None
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x))).cuda()
        return x.to(dtype).contiguous()
    lg, lab = dev(logits, torch.float32), dev(labels, torch.uint8)
    if lg.dim() != 4 or lab.dim() != 3 or lg.shape[:3] != lab.shape or lab.shape[1] != lab.shape[2]:
        raise ValueError("lovasz_grad: logits [B, S, S, K] and labels [B, S, S] expected, got %r and %r" % (tuple(lg.shape), tuple(lab.shape)))
    B, S, K = int(lab.shape[0]), int(lab.shape[1]), int(lg.shape[3])
    lam = P.check_lovasz(lam)
    lm, dc = dev(loss_mask, torch.uint8), dev(dice_coef, torch.float32)
    if lm is not None and lm.shape != lab.shape:
        raise ValueError("lovasz_grad: loss_mask must have the shape of labels")
    if dc is not None and tuple(dc.shape) != (B, K, 2):
        raise ValueError("lovasz_grad: dice_coef must be [B, K, 2]")
    grad, err = torch.empty_like(lg), torch.empty_like(lg)
    rank = torch.empty(lg.shape, dtype=torch.int32, device=lab.device)
    loss = torch.empty(B, dtype=torch.float64, device=lab.device)
    nbytes = _lib.query("drs_lovasz_scratch_bytes", B, S, K)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("drs_patch_lovasz_grad", lg.data_ptr(), err.data_ptr(), lab.data_ptr(), None if lm is None else lm.data_ptr(), B, S, K,
                  lam, None if dc is None else dc.data_ptr(), rank.data_ptr(), grad.data_ptr(), loss.data_ptr(), scratch.data_ptr(), nbytes,
                  torch.cuda.current_stream().cuda_stream)
    return grad, rank.to(torch.int64), err, loss


def hard_mining_weights(logits, labels, keep, min_keep, loss_mask=None, pixel_weight=None):
    """The weight map drs_train_step makes of a step's logits when hard example mining is on, for inspection: logits
    float32 [B, S, S, K] and labels uint8 [B, S, S] (tensors on the GPU, or anything np.asarray takes -- then on the current device),
    loss_mask uint8 [B, S, S] or None, pixel_weight float32 [B, S, S] (the incoming map, e.g. boundary_weight_map's) or None.
    Returns (weights float32 [B, S, S]: 0 where a pixel is left out, n_b / k_b times the incoming weight where it is kept; ce float32
    [B, S, S]: the keys, the plain cross-entropy at in-loss pixels and 0 elsewhere; kept int32 [B]: k_b) as tensors on that device.
    One launch of drs_patch_hard_weight."""
    import torch
    from . import _lib

    def dev(x, dtype):
        if x is None:
            return None
        x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x))).cuda()
        return x.to(dtype).contiguous()
    lg, lab = dev(logits, torch.float32), dev(labels, torch.uint8)
    if lg.dim() != 4 or lab.dim() != 3 or lg.shape[:3] != lab.shape or lab.shape[1] != lab.shape[2]:
        raise ValueError("hard_mining_weights: logits [B, S, S, K] and labels [B, S, S] expected, got %r and %r" % (tuple(lg.shape), tuple(lab.shape)))
    B, S, K = int(lab.shape[0]), int(lab.shape[1]), int(lg.shape[3])
    keep, min_keep = P.check_hard_mining((keep, min_keep))
    lm, pw = dev(loss_mask, torch.uint8), dev(pixel_weight, torch.float32)
    for name, x in (("loss_mask", lm), ("pixel_weight", pw)):
        if x is not None and x.shape != lab.shape:
            raise ValueError("hard_mining_weights: %s must have the shape of labels" % name)
    w = torch.empty(lab.shape, dtype=torch.float32, device=lab.device)
    ce = torch.empty(lab.shape, dtype=torch.float32, device=lab.device)
    kept = torch.empty(B, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("drs_patch_hard_weight", lg.data_ptr(), ce.data_ptr(), lab.data_ptr(), None if lm is None else lm.data_ptr(), B, S, K,
                  keep, min_keep, None if pw is None else pw.data_ptr(), w.data_ptr(), kept.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return w, ce, kept


def boundary_weight_map(labels, valid, a, sigma, R):
    """The weight map drs_train_step makes of a step's labels, for inspection: labels uint8 [B, S, S] (a tensor on the
    GPU, or anything np.asarray takes -- then on the current device), valid the same shape or None.  Returns (weight float32 [B, S, S],
    d2 int32 [B, S, S]: the kernel's uint16 min(D2, 65535), 65535 = no other class within the window) as tensors on the labels' device."""
    from . import _lib
    a, sigma, R = P.check_boundary_weight((a, sigma, R))

    def dev_u8(t, device):
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, dtype=np.uint8)))
        return t.to(device=device, dtype=torch.uint8).contiguous()

    device = labels.device if isinstance(labels, torch.Tensor) and labels.is_cuda else torch.device("cuda", torch.cuda.current_device())
    lab = dev_u8(labels, device)
    if lab.dim() != 3 or lab.shape[1] != lab.shape[2]:
        raise ValueError("labels: expected [B, S, S], got %s" % (tuple(lab.shape),))
    val = None if valid is None else dev_u8(valid, device)
    if val is not None and val.shape != lab.shape:
        raise ValueError("valid: expected the shape of labels, got %s" % (tuple(val.shape),))
    B, S = int(lab.shape[0]), int(lab.shape[1])
    weight = torch.empty((B, S, S), dtype=torch.float32, device=device)
    d2 = torch.empty((B, S, S), dtype=torch.int16, device=device)
    with torch.cuda.device(device):
        _lib.call("drs_patch_boundary_weight", lab.data_ptr(), None if val is None else val.data_ptr(), B, S, R, a,
                  1.0 / (2.0 * sigma * sigma), d2.data_ptr(), weight.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return weight, d2.to(torch.int32) & 0xFFFF


# ------------------------------------------------------------------------------------------------- data parallelism
def sync_rng(comm):
    """Data parallelism runs the same host code on every rank and relies on identical `random` / `numpy.random` streams (size
    draw, batch indices, augmentation).  Nothing guarantees that by itself -- the reference never seeds, and a rank that loads
    a cache file skips the draws the rank that built it made -- so at every point where the ranks may have drifted (start of a
    loop, after a cache was built or loaded) rank 0 draws two seeds from ITS streams and every rank re-seeds from them.
    A single process is untouched (the reference's stream order).
    Returns the pair of seeds: the run seed of whatever keeps a generator of its own (the scale jitter of the training crop,
    patches.draw_scales).  A single process returns the pair rank 0 would have drawn, taken from COPIES of the two streams, so that the
    streams themselves stay where they are."""
    if not getattr(comm, "sync_rng", False):
        r = random.Random()
        r.setstate(random.getstate())
        n = np.random.RandomState()
        n.set_state(np.random.get_state())
        return r.getrandbits(31), int(n.randint(0, 2 ** 31 - 1))
    seeds = comm.broadcast_object((random.getrandbits(31), int(np.random.randint(0, 2 ** 31 - 1))))
    random.seed(seeds[0])
    np.random.seed(seeds[1])
    return int(seeds[0]), int(seeds[1])


def setup_scale_jitter(scale_jitter, seeds, comm, say):
    """The scale jitter of a training run (train's `scale_jitter`; patches.check_scale_jitter) and the run seed of its draws
    (patches.jitter_run_seed of sync_rng's pair): every rank must hold the same ones, asserted once over the ranks.  One log line names
    the range.  Returns ((lo, hi), run seed)."""
    lo, hi = P.check_scale_jitter(scale_jitter)
    run_seed = P.jitter_run_seed(seeds)
    comm.agree([int(np.asarray(lo, dtype=np.float64).view(np.uint64)), int(np.asarray(hi, dtype=np.float64).view(np.uint64)), run_seed],
               "scale jitter")
    say("Scale jitter: every training patch resampled at a scale drawn log-uniformly from [" + "{:.6g}".format(lo) + ", " +
        "{:.6g}".format(hi) + "] (validation and inference at scale 1)")
    return (lo, hi), run_seed


def rank0_call(comm, fn, what):
    """fn() on rank 0 only, its result on every rank.  If rank 0 raises (a bad cache file, an I/O error, a failing builder) EVERY rank
    raises -- the others are not left waiting in the broadcast until the communicator times out."""
    v, err = None, None
    if comm.rank == 0:
        try:
            v = fn()
        except Exception as e:
            if comm.world == 1:
                raise
            err = "%s: %s" % (type(e).__name__, e)
    ok, payload = comm.broadcast_object((err is None, v if err is None else err))
    if not ok:
        raise RuntimeError("rank 0 failed on %s: %s" % (what, payload))
    return payload


def rank0_cached(comm, path, make):
    """the reference's cwd / output .npy caches (isprs:1634-1639, 2087-2115) under data parallelism: rank 0 loads or builds and
    saves, every rank gets rank 0's array (no rank reads a half-written file, every rank takes the same branch)."""
    def load_or_make():
        if os.path.isfile(path):
            return np.load(path, allow_pickle=True)
        v = make()
        tmp = path + ".tmp%d.npy" % os.getpid()
        np.save(tmp, np.asarray(v, dtype=object) if isinstance(v, list) else v)
        os.replace(tmp, path)                    # atomic: a concurrent reader sees the old state or the whole file
        return v
    return rank0_call(comm, load_or_make, path)


# ------------------------------------------------------------------------------------------------- training
class _Pending(object):
    """Results of a step that are read back one step late."""

    def __init__(self, net, out, size_index, step, epoch_counter):
        # pinned destinations: the device-to-host copies are truly asynchronous, the host keeps enqueueing
        self.conf = torch.empty(out["conf"].shape, dtype=out["conf"].dtype, pin_memory=True)
        self.loss_parts = torch.empty(out["loss_parts"].shape, dtype=out["loss_parts"].dtype, pin_memory=True)
        self.conf.copy_(out["conf"], non_blocking=True)
        self.loss_parts.copy_(out["loss_parts"], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        self.size_index, self.step, self.epoch_counter, self.wd = size_index, step, epoch_counter, net.wd

    def get(self):
        self.event.synchronize()
        cm = self.conf.numpy().astype(np.uint32)
        lp = self.loss_parts.numpy()
        return cm, float(lp[0] + self.wd * lp[1])


def train(training_data, training_labels, training_class_distribution, training_rotation_distribution, testing_data,
          testing_labels, testing_class_distribution, testing_instances, lr_initial, batch_size, niter, weight_decay,
          mean_full, std_full, update_type, distribution_type, values, patch_acc_loss, patch_occur, patch_chosen_values,
          probs, resample_batch, output_path, display_step, net_type, dataset, former_model_path=None, *,
          num_classes=6, device="cuda:0", comm=None, noise="device", lr_decay_factor=0.5, tile_dtype=np.float64,
          loss_score_scaled_by_epoch=True, quiet_sizes=False, val_cache_dir=None, class_weights=None, focal_gamma=None,
          scale_jitter=None, boundary_weight=None, dice=None, hard_mining=None, lovasz=None, surface_loss=None):
    """isprs:1621-1851, same positional parameters.  Returns the trained DilatedNet.
    class_weights (opt-in; None = the reference's loss, bit for bit): "balanced" | "median" | K numbers -- per-class weights of the
    cross-entropy (setup_class_weights, DilatedNet.set_class_weights).  The loss this loop prints, and that feeds the size scores with
    update_type="loss", is then the WEIGHTED one (inv_n * sum wc[y] CE + the L2 term); accuracies, confusion matrices and validation
    are not weighted.  Given here, it replaces weights restored from a checkpoint's side file; None keeps those.
    focal_gamma (opt-in; None or 0 = today's run, bit for bit): the focusing parameter of the focal loss, finite in (0, 8]
    (setup_focal_gamma, DilatedNet.set_focal_gamma; with or without class_weights).  The loss this loop prints, and that feeds the
    size scores with update_type="loss", is then the MODULATED one (inv_n * sum wc[y] (1 - p_t)^gamma CE + the L2 term); accuracies,
    confusion matrices and validation are not modulated.  Given here, it replaces a gamma restored from a checkpoint's side file;
    None keeps that.
    boundary_weight (opt-in; None or a = 0 = today's run, bit for bit): (a, sigma, R), or fewer with the defaults of
    patches.check_boundary_weight -- every pixel's loss term and gradient are multiplied by 1 + a exp(-D2 / 2 sigma^2), D2 the squared
    distance to the nearest valid pixel of another class inside the augmented patch (setup_boundary_weight,
    DilatedNet.set_boundary_weight; on top of class_weights and focal_gamma).  The loss this loop prints, and that feeds the size
    scores with update_type="loss", is then the WEIGHTED one: its normaliser is unchanged, so it rises with the mean weight;
    accuracies, confusion matrices and validation are not weighted.  Given here, it replaces a triple restored from a checkpoint's
    side file; None keeps that.  Under data parallelism nothing is added: patches are independent and the normaliser is unchanged.
    dice (opt-in; None or lam = 0 = today's run, bit for bit): (lam, alpha, beta, smooth), or fewer with the defaults of
    patches.check_dice -- a soft Dice / Tversky term per patch is ADDED to the data term (setup_dice, DilatedNet.set_dice; DESIGN.md
    3d), beside whatever form the cross-entropy has: class_weights, focal_gamma and boundary_weight do not weight it.  The loss this
    loop prints, and that feeds the size scores with update_type="loss", is then the cross-entropy part + the Dice term; accuracies,
    confusion matrices and validation do not change.  Given here, it replaces a quadruple restored from a checkpoint's side file; None
    keeps that.  Under data parallelism nothing is added: the soft counts are per patch, and the normaliser is unchanged.
    hard_mining (opt-in; None or keep = 1 = today's run, bit for bit): (keep, min_keep), or keep alone with min_keep = 0 -- online
    hard example mining / bootstrapped cross-entropy (setup_hard_mining, DilatedNet.set_hard_mining): the cross-entropy
    part, in whatever form class_weights, focal_gamma and boundary_weight give it, runs over the max(ceil(keep n_b), min_keep)
    in-loss pixels of every patch with the largest plain cross-entropy at that step, each at the weight n_b / kept; the Dice term is
    not mined.  The loss this loop prints, and that feeds the size scores with update_type="loss", is then the MINED one: the mean of
    the hardest pixels' terms, so it is larger than the loss over all pixels; accuracies, confusion matrices and validation do not
    change.  Given here, it replaces a pair restored from a checkpoint's side file; None keeps that.  Under data parallelism nothing
    is added: the selection is per patch, and the normaliser is unchanged.
    lovasz (opt-in; None or lam = 0 = today's run, bit for bit): lam -- the Lovasz-softmax term per patch, over the classes present in
    it, is ADDED to the data term (setup_lovasz, DilatedNet.set_lovasz), beside whatever form the cross-entropy has:
    class_weights, focal_gamma, boundary_weight and hard_mining do not weight it, and it is not mined.  The loss this loop prints, and
    that feeds the size scores with update_type="loss", is then the cross-entropy part + the Dice term (if on) + the Lovasz term;
    accuracies, confusion matrices and validation do not change.  Given here, it replaces a value restored from a checkpoint's side
    file; None keeps that.  Under data parallelism nothing is added: the order is per patch, and the normaliser is unchanged.
    surface_loss (opt-in; None or lam = 0 = today's run, bit for bit): (lam, clip) -- the boundary (surface) loss per patch, the
    softmax probabilities against lam times the signed distance maps of the patch's labels (clipped to +-clip pixels when clip > 0),
    is ADDED to the data term (setup_surface_loss, DilatedNet.set_surface_loss), beside whatever form the cross-entropy
    has: class_weights, focal_gamma, boundary_weight and hard_mining do not weight it, and it is not mined.  The loss this loop
    prints, and that feeds the size scores with update_type="loss", is then the cross-entropy part + the Dice term (if on) + the
    Lovasz term (if on) + the surface term; accuracies, confusion matrices and validation do not change.  Given here, it replaces a
    pair restored from a checkpoint's side file; None keeps that.  Under data parallelism nothing is added: the maps are per patch,
    and the normaliser is unchanged.
    scale_jitter (opt-in; None = today's run, bit for bit): (lo, hi) -- every training patch is resampled at a scale drawn
    log-uniformly from [lo, hi] (patches.draw_scales, drs_crop_normalize_scaled).  The draws come from a generator of
    their own keyed by (run seed, step), so the sizes, instances and augmentation draws of the run are those of the run without it;
    validation never jitters.  It is not net state: a resumed run is given it again."""
    comm = comm or NoComm()
    say = (lambda *a: print(*a)) if comm.rank == 0 else (lambda *a: None)
    say(BatchColors.OKGREEN + "TRAINING" + BatchColors.ENDC)
    channels = training_data[0].shape[-1]
    say("channels ", channels)

    if batch_size % comm.world:
        raise ValueError("batch_size must be divisible by the number of ranks")
    seeds = sync_rng(comm)       # (the pair from the loop's START is the run seed of the scale jitter: a resumed run, seeded alike, gets
    #                              the same one whether or not the cache below exists by then)
    selected_training_instances = SP.select_super_batch_instances(training_class_distribution, training_rotation_distribution,
                                                                  batch_size, super_batch=SUPER_BATCH)
    total_length = len(selected_training_instances)
    cache = os.path.join(val_cache_dir or os.getcwd(), "dataset_" + dataset + ".npy")      # isprs:1634-1639
    selected_testing_instances = rank0_cached(comm, cache, lambda: SP.select_super_batch_instances(
        testing_class_distribution, batch_size=batch_size, super_batch=SUPER_BATCH))
    sync_rng(comm)                                   # rank 0 may just have drawn what the others did not
    b_local = batch_size // comm.world
    sl = shard_slice(batch_size, comm.rank, comm.world)
    s_max = int(values[0]) if distribution_type == "single_fixed" else int(max(values))
    net = DilatedNet(net_type, channels, num_classes, weight_decay, b_max=b_local, s_max=s_max, device=device, comm=comm,
                     lr_decay_factor=lr_decay_factor)
    train_pool = P.TilePool(training_data, training_labels, device, dtype=tile_dtype)
    test_pool = P.TilePool(testing_data, testing_labels, device, dtype=tile_dtype)
    check_training_labels(train_pool, num_classes)

    shuffle = np.asarray(random.sample(range(total_length), total_length))
    epoch_counter = 1
    current_iter = 1
    sized = distribution_type in ("multi_fixed", "uniform", "multinomial")
    if former_model_path is not None and "model" in former_model_path:
        current_iter = step_from_model_path(former_model_path)
        if sized:
            patch_acc_loss = np.load(output_path + "patch_acc_loss_step_" + str(current_iter) + ".npy")
            patch_occur = np.load(output_path + "patch_occur_step_" + str(current_iter) + ".npy")
            patch_chosen_values = np.load(output_path + "patch_chosen_values_step_" + str(current_iter) + ".npy")
        load_checkpoint(net, former_model_path)
    else:
        say("Model totally initialized!")
    if class_weights is not None:
        setup_class_weights(net, train_pool, num_classes, class_weights, comm, say)
    if focal_gamma is not None:
        setup_focal_gamma(net, focal_gamma, comm, say)
    if boundary_weight is not None:
        setup_boundary_weight(net, boundary_weight, comm, say)
    if dice is not None:
        setup_dice(net, dice, comm, say)
    if hard_mining is not None:
        setup_hard_mining(net, hard_mining, comm, say)
    if lovasz is not None:
        setup_lovasz(net, lovasz, comm, say)
    if surface_loss is not None:
        setup_surface_loss(net, surface_loss, comm, say)
    run_seed = None
    if scale_jitter is not None:
        scale_jitter, run_seed = setup_scale_jitter(scale_jitter, seeds, comm, say)

    it = 0
    epoch_mean = 0.0
    epoch_cm_train = np.zeros((num_classes, num_classes), dtype=np.uint32)
    pending = []
    last = dict(cm=None, loss=None, acc=0)

    def consume(p):
        nonlocal epoch_mean, epoch_cm_train
        cm, loss = p.get()
        acc, _, acc_norm = MT.overall_and_normalized(cm)
        epoch_mean += acc
        epoch_cm_train += cm
        if sized:
            if update_type == "loss":
                patch_acc_loss[p.size_index] += loss * (p.epoch_counter / 10.0) if loss_score_scaled_by_epoch else loss
            else:
                patch_acc_loss[p.size_index] += acc_norm
            patch_occur[p.size_index] += 1
        last.update(cm=cm, loss=loss, acc=acc)

    def flush():
        while pending:
            consume(pending.pop(0))

    step = current_iter
    for step in range(current_iter, niter + 1):
        cur_patch_size, cur_size_int = P.draw_patch_size(distribution_type, values, probs)
        if not quiet_sizes:
            say(cur_patch_size)
        shuffle, batch, it = P.select_batch(shuffle, batch_size, it, total_length)
        if step - current_iter < 3:                  # the ranks must move in lock step: same size, same instances
            comm.agree((cur_patch_size, batch[0], batch[-1], it), "patch size / batch indices at step %d" % step)
        rows = selected_training_instances[batch]
        aug = P.draw_augmentation(rows, cur_patch_size, channels, noise=noise, scale_jitter=scale_jitter,
                                  jitter_key=None if scale_jitter is None else (run_seed, step))
        mine = aug.shard(sl)                             # device noise is keyed by the patch's place in the global batch
        if mine.scale is not None:
            mine.geo = P.scale_geometry(rows[sl], train_pool, cur_patch_size, mine.scale)
        P.crop_to_net(net, train_pool, rows[sl], cur_patch_size, mean_full, std_full, mine)
        out = net.train_step(b_local, cur_patch_size, lr_initial)
        pending.append(_Pending(net, out, cur_size_int, step, epoch_counter))
        while len(pending) > 1:
            consume(pending.pop(0))

        if step != 0 and step % display_step == 0:
            flush()
            cm = last["cm"]
            _, oa, na = MT.overall_and_normalized(cm)
            say("Iter " + str(step) + " -- Time " + str(datetime.datetime.now().time()) +
                " -- Training Minibatch: Loss= " + "{:.6f}".format(last["loss"]) +
                " Absolut Right Pred= " + str(int(last["acc"])) +
                " Overall Accuracy= " + "{:.4f}".format(oa) +
                " Normalized Accuracy= " + "{:.4f}".format(na) +
                " Confusion Matrix= " + _cm_str(cm))

        if step != 0 and step % EPOCH_NUMBER == 0:
            flush()
            _, _, na = MT.overall_and_normalized(epoch_cm_train)
            say("-- Iter " + str(step) + " -- Training Epoch:" +
                " Overall Accuracy= " + "{:.6f}".format(epoch_mean / float(np.sum(epoch_cm_train))) +
                " Normalized Accuracy= " + "{:.6f}".format(na) +
                " Confusion Matrix= " + _cm_str(epoch_cm_train))
            epoch_mean = 0.0
            epoch_cm_train = np.zeros((num_classes, num_classes), dtype=np.uint32)

        if step != 0 and step % VAL_INTERVAL == 0:
            flush()
            if comm.rank == 0:
                save_checkpoint(net, output_path, step, *((patch_acc_loss, patch_occur, patch_chosen_values) if sized else ()))
            cur_patch_val = (select_best_patch_size(distribution_type, values, patch_acc_loss, patch_occur, update_type,
                                                    patch_chosen_values, debug=comm.rank == 0) if sized else int(values[0]))
            validation(net, test_pool, selected_testing_instances, mean_full, std_full, batch_size, step, cur_patch_val, comm)

        if min(it + batch_size, total_length) == total_length or total_length == it + batch_size:     # isprs:1822
            if epoch_counter % resample_batch == 0:
                say("epoch_counter ", epoch_counter)
                selected_training_instances = SP.select_super_batch_instances(training_class_distribution,
                                                                              training_rotation_distribution, batch_size,
                                                                              super_batch=SUPER_BATCH)
                total_length = len(selected_training_instances)
            epoch_counter += 1

    flush()
    say("Optimization Finished!")
    if comm.rank == 0:
        save_checkpoint(net, output_path, step, *((patch_acc_loss, patch_occur, patch_chosen_values) if sized else ()))
    cur_patch_val = (select_best_patch_size(distribution_type, values, patch_acc_loss, patch_occur, update_type,
                                            patch_chosen_values, debug=comm.rank == 0) if sized else int(values[0]))
    validation(net, test_pool, selected_testing_instances, mean_full, std_full, batch_size, step, cur_patch_val, comm)
    return net


# ------------------------------------------------------------------------------------------------- whole tiles
def _check_scores(scores, return_sums):
    """The `scores` argument of an inference path as a tuple of kinds (patches.check_score_kinds), None without it.  Raw sums and scores
    exclude each other: a caller of return_sums finalises itself."""
    if scores is None:
        return None
    kinds = P.check_score_kinds(scores)
    if return_sums:
        raise ValueError("scores and return_sums exclude each other: the score maps are made where the sums are finalised")
    return kinds


def _score_buffers(scores, n, dev):
    """The zeroed uint8 maps, one per kind asked for (patches.check_score_kinds), as a dict in the order asked; None without scores."""
    if scores is None:
        return None
    return {k: torch.zeros(n, dtype=torch.uint8, device=dev) for k in P.check_score_kinds(scores)}


def _check_temperature(temperature_beta, scores, crf=None):
    """The `temperature_beta` argument of an inference path as the float the kernel takes (patches.check_temperature_beta), None without
    it.  A temperature changes the score maps and nothing else, so it needs `scores` -- unless a CRF refines the map (`crf`, DESIGN.md
    8a.6): there it scales the unary, and can change labels."""
    if temperature_beta is None:
        return None
    if scores is None and crf is None:
        raise ValueError("temperature_beta needs score maps (scores / score_maps): a temperature never changes a label")
    return P.check_temperature_beta(temperature_beta)


def _finalize(sums_ptr, occur_ptr, rows, w, K, sums_are_prob, out, smaps, pix0, st, beta=None):
    """Labels of `rows` image rows from their sums (device addresses of the first of those rows) into out[pix0:], by
    drs_stitch_finalize; with score maps (smaps: _score_buffers) by drs_stitch_finalize_scores, which writes the same labels and the
    maps' bytes at the same offset.  sums_are_prob says what the path accumulated and matters to the scores only.
    beta (an inverse temperature, _check_temperature; with smaps only): the maps are drs_stitch_finalize_scores_t's."""
    from . import _lib
    if smaps is None:
        _lib.call("drs_stitch_finalize", sums_ptr, occur_ptr, rows, w, K, out.data_ptr() + pix0, st)
        return
    ptr = [smaps[k].data_ptr() + pix0 if k in smaps else None for k in P.SCORE_KINDS]
    if beta is not None:
        _lib.call("drs_stitch_finalize_scores_t", sums_ptr, occur_ptr, rows, w, K, 1 if sums_are_prob else 0, beta,
                  out.data_ptr() + pix0, ptr[0], ptr[1], ptr[2], st)
        return
    _lib.call("drs_stitch_finalize_scores", sums_ptr, occur_ptr, rows, w, K, 1 if sums_are_prob else 0, out.data_ptr() + pix0,
              ptr[0], ptr[1], ptr[2], st)


def _labels_tail(net, sums, occur, top, row0, rows, h, w, sums_are_prob, scores, beta, comm=None):
    """The tail of every inference path: labels -- and, with `scores` (_check_scores' kinds), score maps -- of image rows
    [row0, row0 + rows) into zeroed [h*w] maps (_finalize), from accumulators whose first element belongs to image row `top`.  With a
    `comm` of several ranks, each of which wrote only the rows it owns, the uint8 maps are gathered by one sum all-reduce each.
    Returns (labels [h, w], {kind: map [h, w]} or None), device tensors."""
    K = net.plan.K
    out = torch.zeros(h * w, dtype=torch.uint8, device=net.dev)
    smaps = _score_buffers(scores, h * w, net.dev)
    if rows > 0:
        d0 = row0 - top
        _finalize(sums.data_ptr() + d0 * w * K * 4, occur.data_ptr() + d0 * w * 4, rows, w, K, sums_are_prob, out, smaps, row0 * w,
                  net._stream(), beta)
    if comm is not None and comm.world > 1:
        comm.all_reduce_sum(out)
        for v in (smaps or {}).values():
            comm.all_reduce_sum(v)
    return out.view(h, w), None if smaps is None else {k: v.view(h, w) for k, v in smaps.items()}


def _public(res, return_sums, scores, count=True):
    """The argument-dependent arity of the public predict_* returns, over the fixed shapes their workers return: (sums, occur, count)
    with return_sums, else (labels, count, score maps or None).  count=False leaves the count out (predict_tile_multiscale has none)."""
    if return_sums:
        return res if count else res[:2]
    labels, n, smaps = res
    out = ((labels, n) if count else (labels,)) + (() if scores is None else (smaps,))
    return out if len(out) > 1 else out[0]


DENSE_SE_MODES = ("global",)


class InferencePath(collections.namedtuple("InferencePath", "crop_size crop_sizes flavour dense_tile dense_tta dense_scales dense_se",
                                           defaults=(None, None, "isprs", None, None, None, None))):
    """Which whole-map inference validate_test, generate_final_maps and fit_temperature run, from their keyword arguments: the sliding
    windows at crop_size (bands of window rows per rank under data parallelism), the multi-size windows (crop_sizes), or overlap-tile
    inference (dense_tile: an int, 0 = the default side) with its dihedral (dense_tta), multi-scale (dense_scales) and whole-image
    squeeze-and-excitation (dense_se) options."""
    __slots__ = ()

    def check(self):
        """ValueError for options that do not go together, or that are malformed; the net is not needed"""
        if self.dense_tile is None:
            if self.dense_tta is not None:
                raise ValueError("test-time augmentation needs overlap-tile inference (dense_tile): the sliding-window map depends on the "
                                 "patch size and has no exact dihedral form")
            if self.dense_scales is not None:
                raise ValueError("multi-scale test-time augmentation needs overlap-tile inference (dense_tile): the sliding windows take "
                                 "their scales from the patch size (crop_sizes)")
            if self.dense_se is not None:
                raise ValueError("whole-image squeeze-and-excitation gates need overlap-tile inference (dense_tile): a sliding window is "
                                 "gated by its own mean")
            return
        if self.dense_tta is not None:
            P.tta_group(self.dense_tta)
        if self.dense_scales is not None:
            P.check_scales(self.dense_scales)
        if self.dense_se is not None and self.dense_se not in DENSE_SE_MODES:
            raise ValueError("dense_se must be one of %s, not %r" % (list(DENSE_SE_MODES), self.dense_se))
        if self.crop_sizes:
            raise ValueError("overlap-tile inference has one scale: its map does not depend on a patch size")

    @property
    def sums_are_prob(self):
        """What the path accumulates per pixel (DESIGN.md 8a.4's table): sums of probability vectors (the multi-size windows; overlap
        tiles with tta or scales) or of logits (the windows and their bands; plain overlap tiles).  The one place that decides it."""
        if self.dense_tile is not None:
            return self.dense_tta is not None or self.dense_scales is not None
        return bool(self.crop_sizes)

    def run(self, net, pool, map_index, batch_size, mean_full, std_full, comm, scores=None, beta=None, return_sums=False):
        """One map through the path.  Returns (labels [h, w], window or tile count -- None for the multi-size windows --, {kind: score
        map} or None); with return_sums (sums [h*w*K], occur [h*w], sums_are_prob), whole on every rank.  scores / beta: as
        _check_scores / _check_temperature return them."""
        worker = _dense if self.dense_tile is not None else _multisize if self.crop_sizes else _window
        res = worker(self, net, pool, map_index, batch_size, mean_full, std_full, comm, scores, beta, return_sums)
        return (res[0], res[1], self.sums_are_prob) if return_sums else res


def predict_tile(net, pool, map_index, crop_size, batch_size, mean_full, std_full, comm=None, return_sums=False, flavour="isprs",
                 scores=None, temperature_beta=None):
    """The inner loop of validate_test / generate_final_maps (isprs:1261-1284, 1925-1949) for one tile: windows at
    stride floor(s/2) (isprs:1243), logits overlap-added in window order, arg-max of the average.  Returns the
    uint8 label map as a DEVICE tensor [h, w].  Under data parallelism batches of windows go round-robin over the
    ranks and the partial sums are added (sum all-reduce of prob / occur).
    scores (opt-in; a tuple of kinds from patches.SCORE_KINDS; not with return_sums): the return value is followed by a dict
    {kind: uint8 device tensor [h, w]} of per-pixel score maps of the averaged logits (drs_stitch_finalize_scores).
    temperature_beta (opt-in; with scores only): the maps are those of softmax(beta x averaged logits); the labels
    do not change."""
    scores = _check_scores(scores, return_sums)
    beta = _check_temperature(temperature_beta, scores)
    return _public(_window(InferencePath(crop_size=crop_size, flavour=flavour), net, pool, map_index, batch_size, mean_full, std_full,
                           comm or NoComm(), scores, beta, return_sums), return_sums, scores)


def _window(path, net, pool, map_index, batch_size, mean_full, std_full, comm, scores, beta, return_sums):
    """predict_tile's worker: (labels, window count, score maps or None), or (prob, occur, window count) with return_sums"""
    from . import _lib
    crop_size, flavour = path.crop_size, path.flavour
    h, w = pool.h[map_index], pool.w[map_index]
    K = net.plan.K
    stride = int(math.floor(crop_size / 2.0))
    n_h, n_w = P.window_counts(h, w, crop_size, stride)
    total = n_h * n_w
    if comm.world > 1 and not return_sums and flavour == "isprs" and n_h >= comm.world:
        labels, smaps = _predict_tile_bands(net, pool, map_index, crop_size, batch_size, mean_full, std_full, comm, scores, beta)
        return labels, total, smaps
    prob = torch.zeros(h * w * K, dtype=torch.float32, device=net.dev)
    occur = torch.zeros(h * w, dtype=torch.int32, device=net.dev)
    # batches are the REFERENCE's: batch i starts where its `batch_size` puts it (for flavour="contest" that start depends on the
    # batch size, contest:275), whatever this net's b_max is -- under data parallelism b_max is batch_size / world -- and is fed
    # to the net in pieces of at most b_max windows
    nb = -(-total // batch_size)
    st = net._stream()
    for i in range(nb):
        if i % comm.world != comm.rank:
            continue
        pos_all = P.window_positions(h, w, crop_size, stride, i, batch_size, flavour)  # flavour: where batch i starts (patches.window_start)
        f0 = P.window_start(h, w, crop_size, stride, i, batch_size, flavour)
        for c0 in range(0, len(pos_all), net.b_max):
            pos = pos_all[c0:c0 + net.b_max]
            inst = np.concatenate([np.full((len(pos), 1), map_index), pos], axis=1)
            P.crop_to_net(net, pool, inst, crop_size, mean_full, std_full)
            _, logits = net.forward(len(pos), crop_size, want_logits=True)
            _lib.call("drs_stitch_accumulate", prob.data_ptr(), occur.data_ptr(), logits.data_ptr(), h, w, K, crop_size, stride, f0 + c0, len(pos), st)
    if comm.world > 1:          # (the multi-scale caller needs the whole sums; the plain path above exchanges bands instead)
        comm.all_reduce_sum(prob)
        comm.all_reduce_sum(occur)
    if return_sums:
        return prob, occur, total
    labels, smaps = _labels_tail(net, prob, occur, 0, 0, h, h, w, path.sums_are_prob, scores, beta)
    return labels, total, smaps


def band_plan(h, crop_size, stride, n_h, world):
    """Window rows per rank and the image rows they touch: rank r takes window rows [a[r], a[r+1]) (contiguous, as even as
    possible); its band is image rows [top[r], bot[r]) (the last window row is shifted back to end at the border, isprs:366-375);
    it OWNS rows [own[r], own[r+1]) of the final map, own[r] = top[r] (own[0] = 0, own[world] = h): what lies below its owned rows
    inside its band is handed to the ranks that own those rows."""
    a = [r * n_h // world for r in range(world + 1)]
    x = lambda i: min(i * stride, h - crop_size)
    top = [x(a[r]) for r in range(world)]
    bot = [x(a[r + 1] - 1) + crop_size for r in range(world)]
    own = [0] + top[1:] + [h]
    return a, top, bot, own


def _predict_tile_bands(net, pool, map_index, crop_size, batch_size, mean_full, std_full, comm, scores=None, beta=None):
    """Sliding-window inference of one tile on several ranks: the window rows are cut into one contiguous band per
    rank, every rank overlap-adds its windows into a band-sized accumulator ([rows of the band][w][K] instead of the whole
    [h][w][K]), only the rows a band shares with the next ranks' territory are exchanged (one sum all-reduce of a buffer in which
    every rank fills its own segment: (world-1) x (S - stride) rows instead of the whole map), each rank divides and arg-maxes the
    rows it owns, and the uint8 label bands are gathered.  Sums are formed as (own windows in window order) + (lower ranks'
    contributions in rank order): deterministic, and equal to the single-rank result up to the association of those float sums.
    scores, beta (_window's): every rank also writes the score maps of the rows it owns, gathered like the labels.
    Returns (labels, {kind: map} or None)."""
    from . import _lib
    h, w = pool.h[map_index], pool.w[map_index]
    K = net.plan.K
    S = crop_size
    stride = int(math.floor(S / 2.0))
    n_h, n_w = P.window_counts(h, w, S, stride)
    W, r = comm.world, comm.rank
    a, top, bot, own = band_plan(h, S, stride, n_h, W)
    rows = bot[r] - top[r]
    prob = torch.zeros(rows * w * K, dtype=torch.float32, device=net.dev)
    occur = torch.zeros(rows * w, dtype=torch.int32, device=net.dev)
    st = net._stream()
    bs = min(batch_size, net.b_max)
    f_end = a[r + 1] * n_w
    # the stitch kernel addresses absolute image rows: hand it the address row 0 would have
    vprob, voccur = prob.data_ptr() - top[r] * w * K * 4, occur.data_ptr() - top[r] * w * 4
    for f0 in range(a[r] * n_w, f_end, bs):
        f = np.arange(f0, min(f0 + bs, f_end))
        pos = np.stack([np.minimum((f // n_w) * stride, h - S), np.minimum((f % n_w) * stride, w - S)], axis=1).astype(np.int64)
        inst = np.concatenate([np.full((len(pos), 1), map_index), pos], axis=1)
        P.crop_to_net(net, pool, inst, S, mean_full, std_full)
        _, logits = net.forward(len(pos), S, want_logits=True)
        _lib.call("drs_stitch_accumulate", vprob, voccur, logits.data_ptr(), h, w, K, S, stride, int(f0), len(pos), st)
    # exchange: segment q of the buffer = rank q's band rows below its owned rows, [own[q+1], bot[q])
    seg = [max(0, bot[q] - own[q + 1]) for q in range(W)]
    off = np.concatenate([[0], np.cumsum(seg)]).astype(np.int64)
    xp = torch.zeros(int(off[-1]) * w * K, dtype=torch.float32, device=net.dev)
    xo = torch.zeros(int(off[-1]) * w, dtype=torch.int32, device=net.dev)
    if seg[r]:
        lo = own[r + 1] - top[r]
        xp[off[r] * w * K:off[r + 1] * w * K].copy_(prob[lo * w * K:(lo + seg[r]) * w * K])
        xo[off[r] * w:off[r + 1] * w].copy_(occur[lo * w:(lo + seg[r]) * w])
    comm.all_reduce_sum(xp)
    comm.all_reduce_sum(xo)
    for q in range(r):          # lower ranks' contributions to the rows this rank owns, in rank order
        lo, hi = max(own[q + 1], own[r]), min(bot[q], own[r + 1])
        if hi > lo:
            src, dst = off[q] + (lo - own[q + 1]), lo - top[r]
            prob[dst * w * K:(dst + hi - lo) * w * K] += xp[src * w * K:(src + hi - lo) * w * K]
            occur[dst * w:(dst + hi - lo) * w] += xo[src * w:(src + hi - lo) * w]
    # every rank finalizes only the rows it owns: the sum all-reduce is the gather of the uint8 bands
    return _labels_tail(net, prob, occur, top[r], own[r], own[r + 1] - own[r], h, w, False, scores, beta, comm)


def predict_tile_multiscale(net, pool, map_index, crop_sizes, batch_size, mean_full, std_full, comm=None, scores=None,
                            temperature_beta=None, return_sums=False):
    """isprs:1347-1474 inner part: for every scale the averaged-logit map, softmax over classes, summed; arg-max.
    scores (predict_tile's): returns (labels, {kind: map}); the maps are of the MEAN of the scales' softmax vectors (the sum divided by
    the number of scales, which leaves the arg-max where it is).  temperature_beta (with scores only): the maps are of
    softmax(beta x log of that mean).  return_sums (not with scores): returns (the summed softmax vectors [h*w*K],
    occur = the number of scales everywhere) instead, on every rank."""
    scores = _check_scores(scores, return_sums)
    beta = _check_temperature(temperature_beta, scores)
    return _public(_multisize(InferencePath(crop_sizes=crop_sizes), net, pool, map_index, batch_size, mean_full, std_full,
                              comm or NoComm(), scores, beta, return_sums), return_sums, scores, count=False)


def _multisize(path, net, pool, map_index, batch_size, mean_full, std_full, comm, scores, beta, return_sums):
    """predict_tile_multiscale's worker: (labels, None, score maps or None), or (acc, occur, None) with return_sums"""
    from . import _lib
    h, w = pool.h[map_index], pool.w[map_index]
    K = net.plan.K
    acc = torch.zeros(h * w * K, dtype=torch.float32, device=net.dev)
    for s_ in path.crop_sizes:
        prob, occur, _ = _window(path._replace(crop_size=int(s_), crop_sizes=None), net, pool, map_index, batch_size, mean_full, std_full,
                                 comm, None, None, True)
        _lib.call("drs_softmax_accumulate", prob.data_ptr(), occur.data_ptr(), h, w, K, acc.data_ptr(), net._stream())
    ones = torch.full((h * w,), 1 if scores is None and not return_sums else len(path.crop_sizes), dtype=torch.int32, device=net.dev)
    if return_sums:
        return acc, ones, None
    labels, smaps = _labels_tail(net, acc, ones, 0, 0, h, h, w, path.sums_are_prob, scores, beta)
    return labels, None, smaps


# ------------------------------------------------------------------------------------------------- whole tiles, overlap-tile
DENSE_TILE = 512        # default tile side of predict_tile_dense (capped by the image's shorter side)
DENSE_BATCH_MAX = 8     # tiles per forward of the inference twin


def dense_batch(plan, T, cap=DENSE_BATCH_MAX):
    """tiles of side T per forward: the largest B <= min(cap, 8) with B*T*T < 2^24 and every activation slab the net lists, and its
    haloed output-gradient slab, below 2^30 floats (include/drs.h conventions; the dense net's 448-channel concat slab binds first)"""
    hmax = max(L.halo for L in plan.layers)
    cmax = max(L.cout for L in plan.layers)
    for b in range(min(int(cap), DENSE_BATCH_MAX), 0, -1):
        if (b * T * T < (1 << 24) and all(b * (T + 2 * P_) ** 2 * C_ < (1 << 30) for C_, P_ in plan.buffers.values())
                and b * (T + 2 * hmax) ** 2 * cmax < (1 << 30)):
            return b
    raise ValueError("dense tile side %d is too large for one forward of %s" % (T, plan.net_type))


def dense_twin(net, T, batch_size):
    """The inference twin of `net` for tiles of side T: a DilatedNet of the same net_type / bands / classes sized (B_t, T), cached on
    `net` (the trained net is sized for its largest training patch, usually far below a tile).  Its parameters and moving statistics
    are copied from `net` device to device on EVERY call (same layout: the same table), so it never lags a net that is still training."""
    B_t = dense_batch(net.plan, T, batch_size)
    twin = getattr(net, "_dense_twin", None)
    if twin is None or (twin.b_max, twin.s_max) != (B_t, T):
        from .engine import EngineNet
        net._dense_twin = None                      # (the old twin's buffers go before the new one's are allocated)
        twin = DilatedNet(net.plan.net_type, net.plan.channels, net.plan.K, net.wd, b_max=B_t, s_max=T, device=net.dev,
                          arith=net.arith, engine=isinstance(net, EngineNet))
        net._dense_twin = twin
    twin.params.copy_(net.params)
    twin.bn.copy_(net.bn)
    return twin


def _se_global_gates(twin, crop, T, boxes, mine, map_index, count, comm, g):
    """The gate sweeps of predict_tile_dense(se="global") for the image transformed by the dihedral code g: for SE
    block j = 0, 1, ... every tile of this rank (`mine`, indices into the plan `boxes`) is cropped transformed by g (crop(inst, g)) and
    forwarded up to the block SE j follows with the gates before it (forward_staged), its activated output summed per channel over the
    tile's core -- as it lies in the transformed tile, patches.dihedral_core_boxes -- into the twin's fp64 se_sum[j], which is zeroed
    on the stream when the sweep begins and summed over the ranks when it ends; se_gate[j] is made of the mean over `count` pixels."""
    local = torch.from_numpy(P.dihedral_core_boxes(boxes, T, g).astype(np.int32)).to(twin.dev)
    for j in range(len(twin.plan.se)):
        twin.se_sum[j].zero_()
        for c0 in range(0, len(mine), twin.b_max):
            sel = mine[c0:c0 + twin.b_max]
            crop(np.concatenate([np.full((len(sel), 1), map_index), boxes[sel, :2]], axis=1), g)
            twin.forward_staged(len(sel), T, j, local.data_ptr() + int(sel[0]) * 6 * 4)
        if comm.world > 1:
            comm.all_reduce_sum(twin.se_sum[j])
        twin.se_gate_finish(j, count)
    twin._keep_boxes = local             # alive until the stream has consumed it


def _tile_pass(twin, T, boxes, n_rows, hg, wg, G, se, prob, occur, comm, crop, map_index):
    """One dense plan over one hg x wg grid (the map, or the map at one scale): this rank's tiles -- a contiguous run of the plan's n_rows
    tile rows, as even as possible over the ranks -- are cropped (crop(inst, g) fills the twin's input slab with the tiles at `inst`
    rows (map, row, col) transformed by the code g: crop_to_net on the plain path, which has no g, crop_dihedral_to_net with tta,
    crop_resampled_to_net with scales), forwarded, and their cores placed into prob / occur [hg][wg]: the logits copied
    (drs_tile_place) without tta (G None), else the softmax mapped back by g^-1 ADDED (drs_tile_place_dihedral).  Without se a batch of
    tiles runs every code of G, ascending (the per-pixel order of the sum); with se every code is a pass of its own over the tiles, after
    its gate sweeps (_se_global_gates).  No collective on prob / occur: that is the caller's.  Returns the split a: rank q took tile
    rows [a[q], a[q+1])."""
    from . import _lib
    K = twin.plan.K
    n_w = len(boxes) // n_rows
    a = [q * n_rows // comm.world for q in range(comm.world + 1)]
    mine = np.arange(a[comm.rank] * n_w, a[comm.rank + 1] * n_w)
    st = twin._stream()
    boxes_dev = torch.from_numpy(boxes.astype(np.int32)).to(twin.dev)
    forward = twin.forward
    if se is not None:
        forward = lambda nb, T_, want_logits: twin.forward_staged(nb, T_, len(twin.plan.se), want_logits=want_logits)   # noqa: E731
    codes = (0,) if G is None else G
    for Gp in ([codes] if se is None else [(g,) for g in codes]):
        if se is not None:
            _se_global_gates(twin, crop, T, boxes, mine, map_index, hg * wg, comm, Gp[0])
        for c0 in range(0, len(mine), twin.b_max):
            sel = mine[c0:c0 + twin.b_max]
            inst = np.concatenate([np.full((len(sel), 1), map_index), boxes[sel, :2]], axis=1)
            box0 = boxes_dev.data_ptr() + int(sel[0]) * 6 * 4
            for g in Gp:
                crop(inst, g)
                _, logits = forward(len(sel), T, want_logits=True)
                if G is None:
                    _lib.call("drs_tile_place", prob.data_ptr(), occur.data_ptr(), logits.data_ptr(), hg, wg, K, T, box0, len(sel), st)
                else:
                    _lib.call("drs_tile_place_dihedral", prob.data_ptr(), occur.data_ptr(), logits.data_ptr(), hg, wg, K, T, box0,
                              len(sel), int(g), st)
    return a


def predict_tile_dense(net, pool, map_index, batch_size, mean_full, std_full, comm=None, tile=None, return_sums=False, tta=None,
                       scales=None, se=None, scores=None, temperature_beta=None):
    """Overlap-tile inference of one tile: the whole-tile forward of the net -- one function of the tile, whatever the patch
    size -- computed exactly in tiles of side T (default min(h, w, 512)).  Every block is stride 1, so an output pixel depends on input
    pixels [p - before, p + after] (nets.Plan.receptive_field); the plan (patches.dense_tiles) gives every tile a core at least that
    margin from every tile edge that is not an image border, and the cores partition the map.  Each tile is cropped and normalised
    (no augmentation), run through the inference twin (dense_twin; batch_size caps its tiles per forward), and its core's logits are
    copied into the map (drs_tile_place); labels by drs_stitch_finalize (occur = 1).  Not the reference's map: no window averaging, no
    window-border padding.  Returns (uint8 labels [h, w] on the device, tile count), or (prob, occur, tile count) with return_sums.
    Data parallelism: rank r takes a contiguous run of tile rows, places its cores into a zeroed map, finalizes the rows its cores own
    and the label maps are gathered by one sum all-reduce (the cores are disjoint); with return_sums prob / occur are summed instead.
    tta ("flip", "d4" or a tuple of codes 0..7; patches.tta_group): dihedral test-time augmentation.  Every tile is run
    once per code g of the group, ascending: cropped transformed by g (drs_crop_dihedral), forwarded, and the softmax of its logits
    mapped back by g^-1 is ADDED into the map (drs_tile_place_dihedral) -- per pixel, the sum over G of softmax(F(g.X)) put back on X's
    grid, occur = |G|; labels the arg-max of that mean.  A flip swaps `before` and `after` on its axis and a transpose swaps the axes,
    so with any g != 0 the plan keeps the symmetric margin max(before, after) on both sides.
    scales (a list of distinct factors in [0.25, 4]; patches.check_scales): multi-scale test-time augmentation, with or
    without tta.  For each scale s, in the order given: the map resampled to hs x ws (patches.scaled_size; bilinear, half-pixel centres)
    is run through the dense plan of side T_s = min(hs, ws, tile or DENSE_TILE) -- each tile cropped from the source map by one fused
    gather (drs_crop_resampled, dihedral code g, 0 without tta), forwarded, and its logits (drs_tile_place) or its per-g softmax
    (drs_tile_place_dihedral) summed into a zeroed hs x ws map; under data parallelism that map is summed over the ranks (the same split
    of tile rows as one scale); then its class probabilities are resampled back onto h x w and ADDED into acc (drs_resample_accumulate)
    on every rank, and the scale's buffers go.  Labels: drs_stitch_finalize(acc, occur = len(scales)) on every rank, which holds the
    whole acc: score maps are made beside them and nothing is gathered.  The tile count is the total over the scales.  One inference
    twin, sized once for max T_s, runs every scale's tiles.
    se ("global"; nets with squeeze-and-excitation blocks only, which raise without it): every SE block scales by the
    sigmoid gate of the mean over ALL h x w pixels of the image -- the function the net computes when the whole image is one patch --
    instead of a patch's own mean (what the window path does, and what training saw: a different function, hence opt-in).  With n
    SE blocks the plan is swept n + 1 times: sweep j forwards every tile up to the block SE j follows with the gates before it and
    sums its activated output over the cores in fp64 (_se_global_gates); the last sweep is the full forward with every gate.  The
    margin is the field with the SE layers as constants (Plan.gated_receptive_field).  The net is not equivariant (asymmetric SAME
    pads, unsymmetric filters), so the activation means of a flipped or rotated image are not those of the image: with tta every
    code g has gates of its own, from sweeps over the g-transformed tiles, before its full forwards; so has every scale, an image of
    its own on its hs x ws grid.
    scores (opt-in; a tuple of kinds from patches.SCORE_KINDS; not with return_sums): the return value is followed by a dict
    {kind: uint8 device tensor [h, w]} of per-pixel score maps (drs_stitch_finalize_scores): of the logits on the plain
    path, of the mean probability vector with tta or scales.  Under data parallelism they are gathered as the labels are.
    temperature_beta (opt-in; with scores only): the maps are of softmax(beta u), u the averaged logits on the plain path and the log of
    the mean probability vector with tta or scales (drs_stitch_finalize_scores_t); the labels do not change."""
    scores = _check_scores(scores, return_sums)
    beta = _check_temperature(temperature_beta, scores)
    path = InferencePath(dense_tile=tile or 0, dense_tta=tta, dense_scales=scales, dense_se=se)
    return _public(_dense(path, net, pool, map_index, batch_size, mean_full, std_full, comm or NoComm(), scores, beta, return_sums),
                   return_sums, scores)


def _dense(path, net, pool, map_index, batch_size, mean_full, std_full, comm, scores, beta, return_sums):
    """predict_tile_dense's worker: (labels, tile count, score maps or None), or (sums, occur, tile count) with return_sums"""
    from . import _lib
    tile, se = path.dense_tile, path.dense_se
    if se is not None and se not in DENSE_SE_MODES:
        raise ValueError("se must be None or one of %s, not %r" % (list(DENSE_SE_MODES), se))
    if se is not None and not net.plan.se:
        raise ValueError("se=%r asks for whole-image squeeze-and-excitation gates, and %s has no squeeze-and-excitation blocks"
                         % (se, net.plan.net_type))
    if se is None and net.plan.receptive_field is None:
        raise ValueError("%s has squeeze-and-excitation blocks (a mean over the whole patch): its output has no finite receptive field, "
                         "so there is no single-pass exact whole-tile inference; use predict_tile, or se=\"global\" for gates from the "
                         "whole image's mean" % net.plan.net_type)
    before, after = net.plan.receptive_field if se is None else net.plan.gated_receptive_field
    G = None if path.dense_tta is None else P.tta_group(path.dense_tta)
    if G is not None and any(G):
        before = after = max(before, after)
    h, w = pool.h[map_index], pool.w[map_index]
    K = net.plan.K
    W, r = comm.world, comm.rank
    if path.dense_scales is None:
        T = int(tile) if tile else min(h, w, DENSE_TILE)
        oy, ys, ye = P.dense_axis(h, T, before, after)
        boxes = P.dense_tiles(h, w, T, before, after)
        twin = dense_twin(net, T, batch_size)
        prob = torch.zeros(h * w * K, dtype=torch.float32, device=net.dev)
        occur = torch.zeros(h * w, dtype=torch.int32, device=net.dev)
        if G is None:
            crop = lambda inst, g: P.crop_to_net(twin, pool, inst, T, mean_full, std_full)                      # noqa: E731
        else:
            crop = lambda inst, g: P.crop_dihedral_to_net(twin, pool, inst, T, mean_full, std_full, g)          # noqa: E731
        a = _tile_pass(twin, T, boxes, len(oy), h, w, G, se, prob, occur, comm, crop, map_index)
        if return_sums:
            if W > 1:
                comm.all_reduce_sum(prob)
                comm.all_reduce_sum(occur)
            return prob, occur, len(boxes)
        # every rank finalizes only the rows its cores own: the sum all-reduce is the gather of the uint8 bands
        own0 = ys[a[r]] if a[r] < len(oy) else h
        own1 = ys[a[r + 1]] if a[r + 1] < len(oy) else h
        labels, smaps = _labels_tail(net, prob, occur, 0, own0, own1 - own0, h, w, path.sums_are_prob, scores, beta, comm)
        return labels, len(boxes), smaps
    one_scale = path._replace(dense_scales=None)         # what a scale's own hs x ws map accumulates
    plans = []
    for s in P.check_scales(path.dense_scales):
        hs, ws = P.scaled_size(h, s), P.scaled_size(w, s)
        T = min(hs, ws, int(tile) if tile else DENSE_TILE)
        if T < max(hs, ws) and T <= before + after:
            raise ValueError("scale %g: the %d x %d map at this scale needs tiles of side %d, which cannot exceed the receptive-field "
                             "margins %d + %d of %s" % (s, hs, ws, T, before, after, net.plan.net_type))
        n_rows = len(P.dense_axis(hs, T, before, after)[0])
        plans.append((hs, ws, T, n_rows, P.dense_tiles(hs, ws, T, before, after)))
    twin = dense_twin(net, max(p[2] for p in plans), batch_size)
    st = twin._stream()
    acc = torch.zeros(h * w * K, dtype=torch.float32, device=net.dev)
    for hs, ws, T, n_rows, boxes in plans:
        prob = torch.zeros(hs * ws * K, dtype=torch.float32, device=net.dev)
        occur = torch.zeros(hs * ws, dtype=torch.int32, device=net.dev)
        crop = lambda inst, g, T=T, hs=hs, ws=ws: P.crop_resampled_to_net(twin, pool, inst, T, hs, ws, mean_full, std_full, g)  # noqa: E731
        _tile_pass(twin, T, boxes, n_rows, hs, ws, G, se, prob, occur, comm, crop, map_index)
        if W > 1:
            comm.all_reduce_sum(prob)
            comm.all_reduce_sum(occur)
        _lib.call("drs_resample_accumulate", prob.data_ptr(), occur.data_ptr(), hs, ws, K, 1 if one_scale.sums_are_prob else 0, h, w,
                  acc.data_ptr(), st)
        del prob, occur          # (stream-ordered: the next scale's buffers may reuse them)
    n_tiles = sum(len(p[4]) for p in plans)
    occur = torch.full((h * w,), len(plans), dtype=torch.int32, device=net.dev)
    if return_sums:
        return acc, occur, n_tiles
    labels, smaps = _labels_tail(net, acc, occur, 0, 0, h, h, w, path.sums_are_prob, scores, beta)
    return labels, n_tiles, smaps


def best_sizes(distribution_type, values, patch_acc_loss, patch_occur, update_type, num_scales):
    """The reference picks the best size, removes it from the candidates and repeats (isprs:1370-1420)."""
    values = np.asarray(values).copy()
    acc, occ = np.asarray(patch_acc_loss).copy(), np.asarray(patch_occur).copy()
    chosen = []
    for _ in range(num_scales):
        if distribution_type not in ("multi_fixed", "uniform", "multinomial"):
            chosen.append(int(values[0]))
            continue
        crop = select_best_patch_size(distribution_type, values, acc, occ, update_type)
        chosen.append(int(crop))
        ind = np.where(values == crop)
        values, acc, occ = np.delete(values, ind), np.delete(acc, ind), np.delete(occ, ind)
    return chosen


def refine_crf(net, pool, map_index, sums, occur, sums_are_prob, crf, scores=None, temperature_beta=None):
    """Local dense-CRF refinement of one map's posterior (opt-in; include/drs.h drs_crf_unary / drs_crf_step): from the
    accumulators an inference path hands out with return_sums (sums [h*w*K], occur [h*w], whole on this rank) and the map's image in
    `pool`, crf.iters mean-field iterations of a bilateral + smoothness Potts model over a (2 radius + 1)^2 window dilated by crf.step
    (crf: what patches.check_crf accepts).  The unary is log softmax(beta u), u the path's score vector (8a.5) and beta =
    temperature_beta (default 1): here a temperature enters the model and CAN change labels.  Two ping-pong Q buffers and the unary,
    4 (3 K + 1) bytes per pixel beside the sums.  Returns (uint8 labels [h, w], {kind: uint8 map [h, w]} or None) as device tensors:
    the first maximum of the refined Q and, with `scores` (kinds from patches.SCORE_KINDS), drs_stitch_finalize_scores' maps of it;
    an uncovered pixel (occur 0) is never a neighbour, keeps label 0 and scores as uncovered."""
    from . import _lib
    crf = P.check_crf(crf)
    kinds = None if scores is None else P.check_score_kinds(scores)
    beta = 1.0 if temperature_beta is None else P.check_temperature_beta(temperature_beta)
    h, w, K, C = pool.h[map_index], pool.w[map_index], net.plan.K, pool.C
    n = h * w
    st = net._stream()
    logp = torch.empty(n * K, dtype=torch.float32, device=net.dev)
    q = [torch.empty(n * K, dtype=torch.float32, device=net.dev) for _ in range(2)]
    live = torch.empty(n, dtype=torch.int32, device=net.dev)
    _lib.call("drs_crf_unary", sums.data_ptr(), occur.data_ptr(), h, w, K, 1 if sums_are_prob else 0, beta, logp.data_ptr(),
              q[0].data_ptr(), live.data_ptr(), st)
    tile = pool.tiles.data_ptr() + int(pool.tile_off[map_index].item()) * (8 if pool.f64 else 4)
    for it in range(crf.iters):
        _lib.call("drs_crf_step", q[it & 1].data_ptr(), logp.data_ptr(), live.data_ptr(), tile, 1 if pool.f64 else 0, C, h, w, K, 0, h,
                  crf.radius, crf.step, crf.w_app, crf.theta_xy, crf.theta_rgb, crf.w_smooth, crf.theta_s, q[(it + 1) & 1].data_ptr(), st)
    return _labels_tail(net, q[crf.iters & 1], live, 0, 0, h, h, w, True, kinds, None)


def _run_path(path, net, pool, k, batch_size, mean_full, std_full, comm, kinds, beta, crf):
    """One map of validate_test / generate_final_maps: (labels, score maps or None) of the path, or, with `crf`, of the CRF that refines
    the path's sums (whole on every rank, so under data parallelism every rank refines the whole map and gets the same bits)."""
    if crf is None:
        pred, _, smaps = path.run(net, pool, k, batch_size, mean_full, std_full, comm, scores=kinds, beta=beta)
        return pred, smaps
    sums, occur, is_prob = path.run(net, pool, k, batch_size, mean_full, std_full, comm, return_sums=True)
    return refine_crf(net, pool, k, sums, occur, is_prob, crf, kinds, beta)


def _calibration_str(cal):
    return ("Calibration ECE= " + "{:.6f}".format(cal["ece"]) + " MCE= " + "{:.6f}".format(cal["mce"]) +
            " Mean Confidence= " + "{:.6f}".format(cal["mean_confidence"]) + " Accuracy= " + "{:.6f}".format(cal["accuracy"]))


def boundary_histogram(truth_dev, pred_dev, h, w, K, ignore_label, distances, hist=None, stream=None):
    """The boundary table of one (truth, prediction) pair of uint8 device maps [h][w] (drs_boundary_histogram; include/drs.h; DESIGN.md
    8a.7): int64 device tensor [(n+1)][(n+1)][K][K], hist[bin in truth][bin in pred][truth][pred], for the distances of
    patches.check_boundary_distances.  `hist` (such a tensor) is ADDED to and returned; without it a zeroed one is made.  stream: a raw
    stream handle (default: torch's current stream on the maps' device).  metrics.boundary_scores turns the table into scores."""
    from . import _lib
    distances = P.check_boundary_distances(distances)
    n = len(distances)
    if hist is None:
        hist = torch.zeros((n + 1, n + 1, K, K), dtype=torch.int64, device=truth_dev.device)
    elif hist.dtype != torch.int64 or tuple(hist.shape) != (n + 1, n + 1, K, K) or not hist.is_contiguous():
        raise ValueError("boundary_histogram: hist must be a contiguous int64 tensor [%d][%d][%d][%d]" % (n + 1, n + 1, K, K))
    if stream is None:
        stream = torch.cuda.current_stream(truth_dev.device).cuda_stream
    dist = (ctypes.c_int * n)(*distances)
    _lib.call("drs_boundary_histogram", truth_dev.data_ptr(), pred_dev.data_ptr(), int(h), int(w), int(K),
              -1 if ignore_label is None else int(ignore_label), ctypes.addressof(dist), n, hist.data_ptr(), stream)
    return hist


def _boundary_str(b):
    """the Boundary line's text from metrics.boundary_scores' dict"""
    bands = b["bands"]
    return ("Boundary d= " + " ".join(str(d) for d in b["distances"]) +
            " Band Pixels= " + " ".join(str(x["count"]) for x in bands) +
            " Band Accuracy= " + " ".join("{:.6f}".format(x["accuracy"]) for x in bands) +
            " Boundary IoU= " + " ".join("{:.6f}".format(x["boundary_iou"]) for x in bands) +
            " Boundary IoU per class (d= " + str(bands[-1]["d"]) + ")= " +
            "[" + " ".join("{:.6f}".format(v) for v in bands[-1]["boundary_iou_per_class"]) + "]" +
            " IoU per class= " + "[" + " ".join("{:.6f}".format(v) for v in b["iou_per_class"]) + "]" +
            " Mean IoU= " + "{:.6f}".format(b["mean_iou"]))


def _on_stream(dev, stream):
    """context in which torch's own operations run on the raw stream handle `stream` (None: torch's current stream on dev, as it is)"""
    # the handle of torch's current stream needs no context -- and must not get one when it is 0, the default stream: an ExternalStream
    # made of a zero handle is a stream from torch's pool instead, unordered with the launches that wrote the caller's maps on stream 0
    if stream is None or stream == torch.cuda.current_stream(dev).cuda_stream:
        return contextlib.nullcontext()
    if stream == 0:
        return torch.cuda.stream(torch.cuda.default_stream(dev))
    return torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev))


def components(map_dev, h, w, connectivity, stream=None):
    """Connected components of a uint8 device map [h][w] (drs_components; include/drs.h): (label, size) as device
    tensors [h, w], label int32 = the smallest linear index y w + x of the pixel's component, size int32 = its pixel count (at most
    2^30), at every pixel.  connectivity 4 or 8.  stream: a raw stream handle (default: torch's current stream on the map's device)."""
    from . import _lib
    if connectivity not in (4, 8):
        raise ValueError("components: connectivity %r, expected 4 or 8" % (connectivity,))
    if map_dev.dtype != torch.uint8 or map_dev.numel() != h * w or not map_dev.is_contiguous():
        raise ValueError("components: the map must be a contiguous uint8 tensor of %d x %d elements" % (h, w))
    with _on_stream(map_dev.device, stream):
        st = torch.cuda.current_stream(map_dev.device).cuda_stream
        label = torch.empty((h, w), dtype=torch.int32, device=map_dev.device)
        size = torch.empty((h, w), dtype=torch.int32, device=map_dev.device)
        _lib.call("drs_components", map_dev.data_ptr(), int(h), int(w), int(connectivity), label.data_ptr(), size.data_ptr(), st)
    return label, size


def sieve_labels(map_dev, h, w, K, sieve, stream=None):
    """The sieve of a uint8 device map [h][w] of K classes (include/drs.h): a minimum mapping unit.  sieve: what
    patches.check_sieve accepts (one threshold or K of them, in pixels; connectivity 4 or 8).  Components (drs_components), then one
    round (drs_sieve_round: every component of a class k below min_size[k] pixels takes the class of its largest 4-neighbouring
    region that is not small itself, ties to the lower class), again until a round merges nothing or patches.SIEVE_MAX_ROUNDS rounds
    have run; the host reads two counters per round.  Bytes >= K never change.  Returns (the sieved map, a new uint8 device tensor
    shaped like map_dev, info) with info = {"rounds": rounds run, the last one, which merged nothing, included; "merged": components
    merged over all rounds; "left_small": small components of the result (0 wherever some component of a class is not small);
    "changed_pixels"; "objects_before" / "objects_after": K component counts each (drs_component_census); "capped": the loop ended at
    SIEVE_MAX_ROUNDS}.  stream: a raw stream handle (default: torch's current stream on the map's device)."""
    from . import _lib
    sieve = P.check_sieve(sieve)
    min_size = P.sieve_thresholds(sieve, K)
    if map_dev.dtype != torch.uint8 or map_dev.numel() != h * w or not map_dev.is_contiguous():
        raise ValueError("sieve_labels: the map must be a contiguous uint8 tensor of %d x %d elements" % (h, w))
    dev, n = map_dev.device, h * w
    host_min = (ctypes.c_int * K)(*min_size)
    with _on_stream(dev, stream):
        st = torch.cuda.current_stream(dev).cuda_stream
        cur = map_dev.clone()
        label = torch.empty(n, dtype=torch.int32, device=dev)
        size = torch.empty(n, dtype=torch.int32, device=dev)
        scratch = torch.empty(_lib.query("drs_sieve_scratch_bytes", int(h), int(w)) // 8, dtype=torch.int64, device=dev)
        counters = torch.empty(2, dtype=torch.int32, device=dev)

        def label_them():
            _lib.call("drs_components", cur.data_ptr(), int(h), int(w), sieve.connectivity, label.data_ptr(), size.data_ptr(), st)

        def objects():
            table = torch.zeros((K, 32), dtype=torch.int64, device=dev)
            _lib.call("drs_component_census", cur.data_ptr(), label.data_ptr(), size.data_ptr(), int(h), int(w), int(K), table.data_ptr(), st)
            return [int(v) for v in table.sum(dim=1).cpu().tolist()]

        def one_round(out):
            _lib.call("drs_sieve_round", cur.data_ptr(), label.data_ptr(), size.data_ptr(), int(h), int(w), int(K),
                      ctypes.addressof(host_min), scratch.data_ptr(), out.data_ptr(), counters.data_ptr(), st)
            return [int(v) for v in counters.cpu().tolist()]
        rounds = merged = 0
        capped = False
        while True:
            label_them()
            if rounds == 0:
                before = objects()
            left, now = one_round(cur)                     # in place
            rounds += 1
            merged += now
            if now == 0:
                break                                      # nothing moved: label and size are those of the result
            if rounds == P.SIEVE_MAX_ROUNDS:
                capped = True
                label_them()
                left = one_round(torch.empty_like(cur))[0]     # counted only: the result is `cur`
                break
        info = {"rounds": rounds, "merged": merged, "left_small": left, "changed_pixels": int((cur != map_dev).sum().item()),
                "objects_before": before, "objects_after": objects(), "capped": capped}
    return cur, info


def _sieve_str(sieve, infos):
    """the Sieve line's text from one sieve_labels info, or from those of all maps (counts summed, the most rounds)"""
    infos = infos if isinstance(infos, list) else [infos]
    total = lambda key: [sum(i[key][k] for i in infos) for k in range(len(infos[0][key]))]
    return ("Sieve min= " + " ".join(str(v) for v in sieve.min_size) + " connectivity= " + str(sieve.connectivity) +
            " Rounds= " + str(max(i["rounds"] for i in infos)) +
            " Merged Components= " + str(sum(i["merged"] for i in infos)) +
            " Changed Pixels= " + str(sum(i["changed_pixels"] for i in infos)) +
            " Objects per class= [" + " ".join(str(v) for v in total("objects_before")) + "] -> [" +
            " ".join(str(v) for v in total("objects_after")) + "]")


def polygons(map_dev, h, w, connectivity=4, stream=None):
    """The polygon outlines of a uint8 device map [h][w] (include/drs.h): every connected region's boundary as closed
    rings on the pixel-corner lattice.  connectivity 4 or 8: what holds a region together (drs_components').  Components, the crack
    count (drs_polygon_count), the rings (drs_polygon_rings, its scratch sized for exactly that count) and the two outputs
    (drs_polygon_write, sized exactly); the host reads the counters in between.  Returns (ring_table, vertices, info): numpy int64
    [rings][7] = (id, label, byte, first vertex, vertex count, crack count, A2), rings by ascending id; numpy int32 [vertices][2] =
    (X, Y), ring after ring; info = {"rings", "exterior" (A2 > 0: one per region), "holes", "vertices", "cracks"}.  A non-zero status
    of either call raises.  stream: a raw stream handle (default: torch's current stream on the map's device)."""
    from . import _lib
    if connectivity not in (4, 8):
        raise ValueError("polygons: connectivity %r, expected 4 or 8" % (connectivity,))
    if not (h >= 1 and w >= 1 and h * w <= 1 << 28):
        raise ValueError("polygons: a map of %d x %d is outside h, w >= 1, h w <= 2^28" % (h, w))
    if map_dev.dtype != torch.uint8 or map_dev.numel() != h * w or not map_dev.is_contiguous():
        raise ValueError("polygons: the map must be a contiguous uint8 tensor of %d x %d elements" % (h, w))
    dev = map_dev.device
    h, w, connectivity = int(h), int(w), int(connectivity)
    with _on_stream(dev, stream):
        st = torch.cuda.current_stream(dev).cuda_stream
        label = torch.empty(h * w, dtype=torch.int32, device=dev)
        size = torch.empty(h * w, dtype=torch.int32, device=dev)
        _lib.call("drs_components", map_dev.data_ptr(), h, w, connectivity, label.data_ptr(), size.data_ptr(), st)
        counters = torch.empty(4, dtype=torch.int64, device=dev)
        _lib.call("drs_polygon_count", map_dev.data_ptr(), h, w, counters.data_ptr(), st)
        cracks = int(counters[0].item())
        scratch = torch.empty(_lib.query("drs_polygon_scratch_bytes", h, w, cracks), dtype=torch.uint8, device=dev)
        _lib.call("drs_polygon_rings", map_dev.data_ptr(), label.data_ptr(), h, w, connectivity, cracks, scratch.data_ptr(),
                  counters.data_ptr(), st)
        got, rings, vertices, status = (int(v) for v in counters.cpu().tolist())
        if status != 0 or got != cracks:
            raise RuntimeError("polygons: drs_polygon_rings status %d with %d cracks for a capacity of %d" % (status, got, cracks))
        table = torch.empty((rings, 7), dtype=torch.int64, device=dev)
        verts = torch.empty((vertices, 2), dtype=torch.int32, device=dev)
        wstatus = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.call("drs_polygon_write", scratch.data_ptr(), h, w, cracks, rings, vertices, table.data_ptr(), verts.data_ptr(),
                  wstatus.data_ptr(), st)
        if int(wstatus.item()) != 0:
            raise RuntimeError("polygons: drs_polygon_write status %d for %d rings, %d vertices" % (int(wstatus.item()), rings, vertices))
        table, verts = table.cpu().numpy(), verts.cpu().numpy()
    exterior = int((table[:, 6] > 0).sum())
    return table, verts, {"rings": rings, "exterior": exterior, "holes": rings - exterior, "vertices": vertices, "cracks": cracks}


_trace_polygons = polygons                  # generate_final_maps' argument of the same name hides the function there


def _polygons_info(table, info, K):
    """what the Polygons line counts of one map: polygons per class (exterior rings of a byte < K), holes of those, their vertices"""
    mine = table[:, 2] < K
    return {"per_class": [int(((table[:, 2] == k) & (table[:, 6] > 0)).sum()) for k in range(K)],
            "holes": int((mine & (table[:, 6] < 0)).sum()), "vertices": int(table[mine, 4].sum()), "cracks": info["cracks"]}


def _polygons_str(connectivity, infos):
    """the Polygons line's text from one map's _polygons_info, or from those of all maps (counts summed)"""
    infos = infos if isinstance(infos, list) else [infos]
    per_class = [sum(i["per_class"][k] for i in infos) for k in range(len(infos[0]["per_class"]))]
    return ("Polygons connectivity= " + str(connectivity) + " Polygons per class= [" + " ".join(str(v) for v in per_class) + "]" +
            " Holes= " + str(sum(i["holes"] for i in infos)) + " Vertices= " + str(sum(i["vertices"] for i in infos)))


def superpixel_scale(pool, map_index):
    """(lo, inv) of drs_superpixel_features for one map of the pool, two float32 numpy arrays [C]: per channel lo = the map's own
    minimum and inv = 255 / (max - min) in fp32, 0 where max == min -- the bytes span what the map holds, whatever its units.  The
    minimum and maximum are torch's (aminmax over the tile view, on the current stream); this reads them back."""
    h, w, C = pool.h[map_index], pool.w[map_index], pool.C
    off = int(pool.tile_off[map_index].item())
    lo, hi = torch.aminmax(pool.tiles[off:off + h * w * C].view(h * w, C), dim=0)
    lo, hi = lo.cpu().numpy().astype(np.float32), hi.cpu().numpy().astype(np.float32)      # rounding is monotonic: min and max of the fp32 values
    with np.errstate(all="ignore"):
        inv = np.where(hi == lo, np.float32(0), np.float32(255) / (hi - lo)).astype(np.float32)
    return lo, inv


def superpixels(pool, map_index, params, stream=None):
    """The superpixels of one map's image in `pool` (include/drs.h): byte features at the map's own scale
    (superpixel_scale, drs_superpixel_features), integer SLIC on them (drs_superpixels; params: what patches.check_superpixel accepts)
    and the connected pieces of the clusters (drs_components on the 16-colouring, connectivity 4).  Returns (assign, region_label,
    region_size, centres) as device tensors: assign int32 [h, w] = the centre id of every pixel; region_label int32 [h, w] = the
    smallest linear index of the pixel's region; region_size int32 [h, w]; centres int32 [gh gw, C + 3] = (cx, cy, features, pixel
    count).  stream: a raw stream handle (default: torch's current stream on the pool's device)."""
    from . import _lib
    params = P.check_superpixel(params)
    h, w, C = pool.h[map_index], pool.w[map_index], pool.C
    need = _lib.query("drs_superpixel_scratch_bytes", C, h, w, params.size)
    if need == 0:
        raise ValueError("superpixels: a map of %d x %d x %d is outside 1 <= h, w <= 32768, 1 <= C <= 8" % (h, w, C))
    dev = pool.tiles.device
    with _on_stream(dev, stream):
        st = torch.cuda.current_stream(dev).cuda_stream
        lo, inv = superpixel_scale(pool, map_index)
        tile = pool.tiles.data_ptr() + int(pool.tile_off[map_index].item()) * (8 if pool.f64 else 4)
        feat = torch.empty((h, w, C), dtype=torch.uint8, device=dev)
        _lib.call("drs_superpixel_features", tile, 1 if pool.f64 else 0, C, h, w, lo.ctypes.data, inv.ctypes.data, feat.data_ptr(), st)
        ncentres = need // (4 * (C + 3))
        assign = torch.empty((h, w), dtype=torch.int32, device=dev)
        colour = torch.empty((h, w), dtype=torch.uint8, device=dev)
        centres = torch.empty((ncentres, C + 3), dtype=torch.int32, device=dev)
        scratch = torch.empty(need // 4, dtype=torch.int32, device=dev)
        _lib.call("drs_superpixels", feat.data_ptr(), C, h, w, params.size, params.compactness, params.iters, assign.data_ptr(),
                  colour.data_ptr(), centres.data_ptr(), scratch.data_ptr(), st)
        label = torch.empty((h, w), dtype=torch.int32, device=dev)
        size = torch.empty((h, w), dtype=torch.int32, device=dev)
        _lib.call("drs_components", colour.data_ptr(), h, w, 4, label.data_ptr(), size.data_ptr(), st)
    return assign, label, size, centres


def region_vote(map_dev, label, h, w, K, weight=None, stream=None):
    """The vote of a uint8 device map [h][w] of K classes inside the regions of `label` (drs_region_vote; include/drs.h; DESIGN.md
    8a.11): label int32 [h][w] = the smallest linear index of every pixel's region, as drs_components writes it -- any such labelling.
    Every region takes the class with the largest sum of `weight` (a uint8 device map [h][w]; None: 1 per pixel) over its pixels,
    ties to the lower class; a region whose largest sum is 0 stays as it is; bytes >= K neither vote nor change.  Returns (the voted
    map, a new uint8 device tensor shaped like map_dev, info) with info = {"regions", "changed_pixels"}; reading the two counters is
    the one synchronisation.  stream: a raw stream handle (default: torch's current stream on the map's device)."""
    from . import _lib
    _byte_map("region_vote", "map", map_dev, h, w)
    if label.dtype != torch.int32 or label.numel() != h * w or not label.is_contiguous():
        raise ValueError("region_vote: the labels must be a contiguous int32 tensor of %d x %d elements" % (h, w))
    if weight is not None:
        _byte_map("region_vote", "weight", weight, h, w)
    need = _lib.query("drs_region_vote_scratch_bytes", int(h), int(w))
    if need == 0:
        raise ValueError("region_vote: a map of %d x %d is outside 1 <= h, w <= 32768" % (h, w))
    dev = map_dev.device
    with _on_stream(dev, stream):
        st = torch.cuda.current_stream(dev).cuda_stream
        out = torch.empty_like(map_dev)
        scratch = torch.empty(need // 8, dtype=torch.int64, device=dev)
        counters = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.call("drs_region_vote", map_dev.data_ptr(), label.data_ptr(), None if weight is None else weight.data_ptr(), int(h), int(w),
                  int(K), scratch.data_ptr(), out.data_ptr(), counters.data_ptr(), st)
        regions, changed = [int(v) for v in counters.cpu().tolist()]
    return out, {"regions": regions, "changed_pixels": changed}


def superpixel_vote(net, pool, map_index, pred, params, confidence=None):
    """Object-based voting of one map (opt-in): the superpixels of the map's image (superpixels) and the vote of the
    label map `pred` (uint8 device [h, w]) inside their connected pieces (region_vote), on the net's stream.  params: what
    patches.check_superpixel accepts; with weight "confidence" a pixel votes with its byte of `confidence` (the path's uint8
    confidence map), else once.  Returns (the voted map, info) with info = {"regions", "changed_pixels", "centres"}."""
    params = P.check_superpixel(params)
    if params.weight == "confidence" and confidence is None:
        raise ValueError("superpixel_vote: weight 'confidence' needs the path's confidence map")
    h, w, st = pool.h[map_index], pool.w[map_index], net._stream()
    _, label, _, centres = superpixels(pool, map_index, params, stream=st)
    out, info = region_vote(pred, label, h, w, net.plan.K, weight=confidence if params.weight == "confidence" else None, stream=st)
    return out, dict(info, centres=int(centres.shape[0]))


def _superpixel_str(params, infos):
    """the Superpixel line's text from one superpixel_vote info, or from those of all maps (counts summed)"""
    infos = infos if isinstance(infos, list) else [infos]
    return ("Superpixel size= " + str(params.size) + " compactness= " + str(params.compactness) + " iters= " + str(params.iters) +
            " weight= " + params.weight + " Regions= " + str(sum(i["regions"] for i in infos)) +
            " Changed Pixels= " + str(sum(i["changed_pixels"] for i in infos)))


def object_table(truth_dev, pred_dev, h, w, K, ignore_label, connectivity, table=None, stream=None):
    """The object table of one (truth, prediction) pair of uint8 device maps [h][w] (include/drs.h): the connected
    components of both maps at `connectivity` (two drs_components), the match of the two labellings (drs_object_match: a truth object
    and a predicted object of the same class match iff their IoU exceeds 1/2, pixels over ignored truth aside) and the counts
    (drs_object_table): int64 device tensor [K][4][32], by floor(log2(size)): truth objects, predicted objects, matched truth
    objects, the sum of floor(IoU 2^20) over them.  `table` (such a tensor) is ADDED to and returned, so the maps of a split
    accumulate; without it a zeroed one is made.  ignore_label: None or -1 for none.  stream: a raw stream handle (default: torch's
    current stream on the maps' device); everything, the zeroing of a new table included, is enqueued there and nothing waits: a
    caller that names a stream orders its own reads of the table after it.  metrics.object_scores turns the table into scores."""
    from . import _lib
    connectivity = P.check_object_scores(connectivity)
    for name, m in (("truth", truth_dev), ("prediction", pred_dev)):
        if m.dtype != torch.uint8 or m.numel() != h * w or not m.is_contiguous():
            raise ValueError("object_table: the %s must be a contiguous uint8 tensor of %d x %d elements" % (name, h, w))
    dev, n = truth_dev.device, h * w
    if table is not None and (table.dtype != torch.int64 or tuple(table.shape) != (K, 4, 32) or not table.is_contiguous()):
        raise ValueError("object_table: table must be a contiguous int64 tensor [%d][4][32]" % K)
    ignore = -1 if ignore_label is None else int(ignore_label)
    with _on_stream(dev, stream):
        st = torch.cuda.current_stream(dev).cuda_stream
        if table is None:
            table = torch.zeros((K, 4, 32), dtype=torch.int64, device=dev)
        tlabel, tsize, plabel, psize, match, inter, cover = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(7)]
        scratch = torch.empty(_lib.query("drs_object_scratch_bytes", int(h), int(w)) // 8, dtype=torch.int64, device=dev)
        _lib.call("drs_components", truth_dev.data_ptr(), int(h), int(w), connectivity, tlabel.data_ptr(), tsize.data_ptr(), st)
        _lib.call("drs_components", pred_dev.data_ptr(), int(h), int(w), connectivity, plabel.data_ptr(), psize.data_ptr(), st)
        _lib.call("drs_object_match", truth_dev.data_ptr(), pred_dev.data_ptr(), tlabel.data_ptr(), tsize.data_ptr(), plabel.data_ptr(),
                  psize.data_ptr(), int(h), int(w), int(K), ignore, scratch.data_ptr(), match.data_ptr(), inter.data_ptr(), cover.data_ptr(), st)
        _lib.call("drs_object_table", truth_dev.data_ptr(), tlabel.data_ptr(), tsize.data_ptr(), pred_dev.data_ptr(), plabel.data_ptr(),
                  psize.data_ptr(), match.data_ptr(), inter.data_ptr(), cover.data_ptr(), int(h), int(w), int(K), ignore, table.data_ptr(), st)
    return table


def _objects_str(connectivity, o):
    """the Objects line's text from metrics.object_scores' dict"""
    ints = lambda v: "[" + " ".join(str(int(x)) for x in v) + "]"
    vals = lambda v: "[" + " ".join("{:.6f}".format(x) for x in v) + "]"
    return ("Objects connectivity= " + str(connectivity) + " Truth= " + ints(o["truth"]) + " Predicted= " + ints(o["predicted"]) +
            " Matched= " + ints(o["matched"]) + " Precision= " + vals(o["precision"]) + " Recall= " + vals(o["recall"]) +
            " F1= " + vals(o["f1"]) + " SQ= " + vals(o["sq"]) + " PQ= " + vals(o["pq"]) +
            " Mean F1= " + "{:.6f}".format(o["mean_f1"]) + " Mean SQ= " + "{:.6f}".format(o["mean_sq"]) +
            " Mean PQ= " + "{:.6f}".format(o["mean_pq"]) + " All Objects F1= " + "{:.6f}".format(o["all"]["f1"]) +
            " SQ= " + "{:.6f}".format(o["all"]["sq"]) + " PQ= " + "{:.6f}".format(o["all"]["pq"]))


DT_MODES = {"class": 0, "not_class": 1, "contour": 2}          # DRS_DT_* of include/drs.h


def _byte_map(name, what, m, h, w):
    if m.dtype != torch.uint8 or m.numel() != h * w or not m.is_contiguous():
        raise ValueError("%s: the %s must be a contiguous uint8 tensor of %d x %d elements" % (name, what, h, w))


def distance_transform(map_dev, h, w, mode, cls, veil=None, veil_label=None, stream=None):
    """The exact squared Euclidean distance transform of a uint8 device map [h][w] (drs_distance_transform; include/drs.h; DESIGN.md
    8a.10): int32 device tensor [h, w], the squared distance of every pixel to the nearest site, 0x7fffffff everywhere without a site;
    no window.  mode: 0 / "class" (sites: byte == cls), 1 / "not_class" (byte != cls), 2 / "contour" (byte == cls with a 4-neighbour
    inside the map of another byte).  veil (a uint8 device map [h][w]) with veil_label: the byte read is veil_label wherever the veil
    carries it.  h, w <= 32768, h w <= 2^28.  stream: a raw stream handle (default: torch's current stream on the map's device)."""
    from . import _lib
    mode = DT_MODES.get(mode, mode)
    if isinstance(mode, bool) or mode not in (0, 1, 2):
        raise ValueError("distance_transform: mode %r, expected 0..2 or one of %s" % (mode, ", ".join(sorted(DT_MODES))))
    _byte_map("distance_transform", "map", map_dev, h, w)
    if (veil is None) != (veil_label is None):
        raise ValueError("distance_transform: veil and veil_label go together")
    if veil is not None:
        _byte_map("distance_transform", "veil", veil, h, w)
    need = _lib.query("drs_distance_scratch_bytes", int(h), int(w))
    if need == 0:
        raise ValueError("distance_transform: a map of %d x %d is outside 1 <= h, w <= 32768, h w <= 2^28" % (h, w))
    dev = map_dev.device
    with _on_stream(dev, stream):
        st = torch.cuda.current_stream(dev).cuda_stream
        d2 = torch.empty((h, w), dtype=torch.int32, device=dev)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.call("drs_distance_transform", map_dev.data_ptr(), None if veil is None else veil.data_ptr(),
                  0 if veil_label is None else int(veil_label), int(h), int(w), mode, int(cls), d2.data_ptr(), scratch.data_ptr(), need, st)
    return d2


def surface_histogram(truth_dev, pred_dev, h, w, K, ignore_label, table=None, stream=None):
    """The surface-distance table of one (truth, prediction) pair of uint8 device maps [h][w] (drs_surface_histogram; include/drs.h;
    DESIGN.md 8a.10): int64 device tensor [2][K][metrics.SURFACE_BINS + 2]: per direction (0: the truth's contour pixels against the
    prediction's contour, 1: the reverse) and class, the pixels by ceil(4 distance), the sum of floor(1024 distance) and the pixels
    whose counterpart contour is empty.  `table` (such a tensor) is ADDED to and returned, so the maps of a split accumulate; without
    it a zeroed one is made.  ignore_label: None or -1 for none.  stream: a raw stream handle (default: torch's current stream on the
    maps' device); everything is enqueued there and nothing waits.  metrics.surface_scores turns the table into scores."""
    from . import _lib
    _byte_map("surface_histogram", "truth", truth_dev, h, w)
    _byte_map("surface_histogram", "prediction", pred_dev, h, w)
    shape = (2, K, MT.SURFACE_BINS + 2)
    if table is not None and (table.dtype != torch.int64 or tuple(table.shape) != shape or not table.is_contiguous()):
        raise ValueError("surface_histogram: table must be a contiguous int64 tensor [2][%d][%d]" % (K, shape[2]))
    need = _lib.query("drs_surface_scratch_bytes", int(h), int(w))
    if need == 0:
        raise ValueError("surface_histogram: a map of %d x %d is outside 1 <= h, w <= 32768, h w <= 2^28" % (h, w))
    dev = truth_dev.device
    with _on_stream(dev, stream):
        st = torch.cuda.current_stream(dev).cuda_stream
        if table is None:
            table = torch.zeros(shape, dtype=torch.int64, device=dev)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.call("drs_surface_histogram", truth_dev.data_ptr(), pred_dev.data_ptr(), int(h), int(w), int(K),
                  -1 if ignore_label is None else int(ignore_label), table.data_ptr(), scratch.data_ptr(), need, st)
    return table


def _surface_str(s):
    """the Surface line's text from metrics.surface_scores' dict"""
    ints = lambda v: "[" + " ".join(str(int(x)) for x in v) + "]"
    vals = lambda v: "[" + " ".join("{:.6f}".format(x) for x in v) + "]"
    return ("Surface tau= " + " ".join(str(t) for t in s["tolerances"]) + " Truth Contour= " + ints(s["n_truth"]) +
            " Predicted Contour= " + ints(s["n_pred"]) + " Unsited= " + ints(s["unsited_truth"]) + " " + ints(s["unsited_pred"]) +
            " ASSD= " + vals(s["assd"]) + " HD95= " + vals(s["hd95"]) + " Saturated= " + ints(s["saturated"]) +
            " HD100= " + vals(s["hd100"]) + " NSD= " + " ".join(vals(row) for row in s["nsd"]) +
            " Mean ASSD= " + "{:.6f}".format(s["mean_assd"]) + " Mean HD95= " + "{:.6f}".format(s["mean_hd95"]) +
            " Mean NSD= " + " ".join("{:.6f}".format(v) for v in s["mean_nsd"]))


FIT_RESIDENT_BYTES = 32 << 30       # default cap on the accumulators fit_temperature keeps on the device


def fit_temperature(net, testing_data, testing_labels, batch_size, mean_full, std_full, crop_size, comm=None, pool=None, ignore_label=6,
                    crop_sizes=None, flavour="isprs", dense_tile=None, dense_tta=None, dense_scales=None, dense_se=None,
                    max_resident_bytes=FIT_RESIDENT_BYTES, lo=P.BETA_MIN, hi=P.BETA_MAX, max_iter=60):
    """Fit the one scalar of temperature scaling on labelled maps, for the inference path the arguments name (those of
    validate_test).  One inference pass: per map the path's own accumulators (return_sums: the whole sums and occur on every rank) stay
    on the device, 4 (K + 1) bytes per pixel; a split that needs more than max_resident_bytes raises ValueError, naming the need.  Then
    metrics.fit_temperature, every evaluation one drs_temperature_stats launch per map into one zeroed [5], in the mode the path
    accumulates in (8a.4's table; occur = len(crop_sizes) for the multi-size windows).  The counted pixels are the confusion matrix's,
    less the uncovered ones.  Under data parallelism every rank computes the same statistics; the ranks check that they agree on
    beta's float32 bits (comm.agree), no other collective is added.  Returns metrics.fit_temperature's dict, beta rounded to the
    float32 the kernels take."""
    from . import _lib
    comm = comm or NoComm()
    path = InferencePath(crop_size, crop_sizes, flavour, dense_tile, dense_tta, dense_scales, dense_se)
    path.check()
    if testing_labels is None and pool is None:
        raise ValueError("fit_temperature needs labelled maps")
    K = net.plan.K
    pool = pool or P.TilePool(testing_data, testing_labels, net.dev)
    need = sum(4 * (K + 1) * pool.h[k] * pool.w[k] for k in range(len(testing_data)))
    if need > max_resident_bytes:
        raise ValueError("fit_temperature keeps the accumulators of the whole split on the device: %d bytes (4 (K + 1) per pixel) "
                         "exceed max_resident_bytes = %d" % (need, max_resident_bytes))
    kept = []
    for k in range(len(testing_data)):
        sums, occur, is_prob = path.run(net, pool, k, batch_size, mean_full, std_full, comm, return_sums=True)
        n = pool.h[k] * pool.w[k]
        off = int(pool.lab_off[k].item())
        kept.append((sums, occur, pool.labels[off:off + n], n, 1 if is_prob else 0))
    st = net._stream()
    scratch = torch.zeros(max([1] + [_lib.query("drs_temperature_scratch_doubles", q[3]) for q in kept]), dtype=torch.float64, device=net.dev)

    def stats_fn(beta):
        out = torch.zeros(5, dtype=torch.float64, device=net.dev)
        for sums, occur, lab, n, is_prob in kept:
            _lib.call("drs_temperature_stats", sums.data_ptr(), occur.data_ptr(), lab.data_ptr(), n, K, is_prob, ignore_label,
                      float(beta), scratch.data_ptr(), out.data_ptr(), st)
        return out.cpu().tolist()
    fit = MT.fit_temperature(stats_fn, lo=lo, hi=hi, max_iter=max_iter)
    fit["beta"] = P.check_temperature_beta(fit["beta"])
    fit["temperature"] = 1.0 / fit["beta"]
    comm.agree([int(np.float32(fit["beta"]).view(np.uint32))], "the fitted inverse temperature")
    return fit


def validate_test(net, testing_data, testing_labels, testing_instances, batch_size, mean_full, std_full, crop_size, step,
                  output_path=None, comm=None, pool=None, ignore_label=6, crop_sizes=None, flavour="isprs", dense_tile=None,
                  dense_tta=None, dense_scales=None, dense_se=None, score_maps=None, temperature_beta=None, crf=None,
                  boundary_scores=None, sieve=None, surface_scores=None, superpixel=None, object_scores=None):
    """isprs:1241-1344: per tile, sliding-window prediction and scores (label 6 = eroded boundary is skipped,
    isprs:1294).  Returns (all-maps confusion matrix, list of label maps as numpy).  dense_tile (an int, 0 = the default side): the
    maps come from overlap-tile inference (predict_tile_dense) instead of the windows; the scores are computed as before.  dense_tta
    ("flip", "d4" or a tuple of codes; with dense_tile only): its dihedral test-time augmentation (predict_tile_dense's tta).
    dense_scales (a list of factors; with dense_tile only): its multi-scale test-time augmentation (predict_tile_dense's scales).
    dense_se ("global"; with dense_tile only, nets with squeeze-and-excitation blocks): its whole-image gates (predict_tile_dense's se).
    score_maps (opt-in; a tuple of kinds from patches.SCORE_KINDS; any inference path): per-pixel score maps beside the labels and a
    calibration report.  "confidence" is computed whether asked for or not: the report needs it.  Per map, and for all
    maps, one line `---- Iter N -- Test Map M: Calibration ECE= ... MCE= ... Mean Confidence= ... Accuracy= ...` follows the
    reference-format line, which stays as it is; the pixels are those the confusion matrix counts.  Returns (all-maps confusion
    matrix, label maps, extra) with extra = {"scores": [per map {kind: uint8 numpy [h, w]}], "reliability": the all-maps table
    [256][2] (drs_reliability_histogram), "calibration": metrics.calibration of it, plus "per_map": [the same per map]}.
    temperature_beta (opt-in; with score_maps only; an inverse temperature, e.g. fit_temperature's): the score maps, and so the
    calibration report, are of the calibrated probabilities; every Calibration line then ends in ` Temperature= T`
    (T = 1 / beta) and extra carries "temperature_beta".  Labels and reference-format lines do not change.
    crf (opt-in; any inference path; what patches.check_crf accepts): every map is the path's posterior refined by a local dense CRF
    against the image (refine_crf): accuracy, kappa, confusion matrix, returned maps, score maps and calibration
    lines are then those of the refined map.  With crf a temperature_beta is accepted without score_maps: it scales the unary, so
    with a CRF it CAN change labels.  Without crf nothing changes.
    boundary_scores (opt-in; any inference path; a tuple of distances in pixels, patches.check_boundary_distances, e.g.
    patches.BOUNDARY_DEFAULT): trimap accuracy, Boundary IoU and plain IoU of every map and of all maps: per map, one
    drs_boundary_histogram call on the labels and the map that drs_confusion scored -- the refined map with crf.  One line
    `---- Iter N -- Test Map M: Boundary d= ... Band Pixels= ... Band Accuracy= ... Boundary IoU= ... Boundary IoU per class (d= D)= ...
    IoU per class= ... Mean IoU= ...` follows the reference-format line (and the Calibration line where there is one), per map and
    for all maps from the summed table.  Returns (all-maps confusion matrix, label maps, extra) with extra["boundary"] =
    metrics.boundary_scores of the all-maps table, plus "per_map": [the same per map] and "hist": the int64 numpy table; the score-map
    keys are in extra only when score_maps is given too.  Without boundary_scores nothing changes.
    sieve (opt-in; any inference path; what patches.check_sieve accepts: one threshold in pixels or one per class, and a
    connectivity): a minimum mapping unit (sieve_labels).  The map the path returns -- the refined map with crf -- is
    sieved before anything scores it: confusion matrix, accuracy, F1, kappa, the boundary scores and the returned maps are those of
    the sieved map.  Score maps and Calibration lines describe the posterior and stay those of the UNSIEVED labels: a sieved pixel's
    label is no longer its winning class.  Every rank sieves the whole map itself and gets the same bits.  One line
    `---- Iter N -- Test Map M: Sieve min= ... connectivity= c Rounds= r Merged Components= n Changed Pixels= p Objects per class=
    [before] -> [after]` follows the map's other lines, and one for all maps (counts summed, the most rounds) the all-maps lines.
    Returns (all-maps confusion matrix, label maps, extra) with extra["sieve"] = {"params": the SieveParams, "per_map": [sieve_labels'
    info per map], "rounds" (the most), "merged", "changed_pixels", "left_small", "objects_before", "objects_after" (summed)}.  Without
    sieve nothing changes.
    object_scores (opt-in; any inference path; a connectivity, 4 or 8, patches.check_object_scores): object-level scores of every map
    and of all maps: per map, one object_table call on the labels and the map that drs_confusion scored -- the sieved
    refined map with crf / sieve --, with the ignore label the boundary scores pass; the connected regions of each class are the
    objects, a truth object and a predicted one match iff their IoU exceeds 1/2.  Every rank scores the whole map itself and gets the
    same bits.  One line `---- Iter N -- Test Map M: Objects connectivity= c Truth= [..] Predicted= [..] Matched= [..] Precision= [..]
    Recall= [..] F1= [..] SQ= [..] PQ= [..] Mean F1= ... Mean SQ= ... Mean PQ= ... All Objects F1= ... SQ= ... PQ= ...` follows the
    map's other lines, and one for all maps, from the summed table, the all-maps lines.  Returns (all-maps confusion matrix, label
    maps, extra) with extra["objects"] = metrics.object_scores of the all-maps table, plus "connectivity", "table" (the int64 numpy
    table [K][4][32]) and "per_map": [the same per map, each with its "table"].  Without object_scores nothing changes.
    surface_scores (opt-in; any inference path; a tuple of tolerances in pixels, patches.check_surface_tolerances, e.g.
    patches.SURFACE_DEFAULT): surface-distance scores of every map and of all maps: per map, one surface_histogram
    call on the labels and the map that drs_confusion scored -- the sieved refined map with crf / sieve --, with the ignore label the
    boundary scores pass; the distances are exact and unbounded.  Every rank scores the whole map itself and gets the same bits; no
    collective is added.  One line `---- Iter N -- Test Map M: Surface tau= ... Truth Contour= [..] Predicted Contour= [..] Unsited=
    [..] [..] ASSD= [..] HD95= [..] Saturated= [..] HD100= [..] NSD= [..] ... Mean ASSD= ... Mean HD95= ... Mean NSD= ...` follows the
    map's other lines, and one for all maps, from the summed table, the all-maps lines.  Returns (all-maps confusion matrix, label
    maps, extra) with extra["surface"] = metrics.surface_scores of the all-maps table, plus "table" (the int64 numpy table [2][K][4098])
    and "per_map": [the same per map, each with its "table"].  Without surface_scores nothing changes.
    superpixel (opt-in; any inference path; what patches.check_superpixel accepts: size, compactness, iters, weight): object-based
    voting (superpixel_vote).  The map the path returns -- the refined map with crf -- is voted inside the connected
    pieces of the superpixels of the map's image BEFORE the sieve and before anything scores it; the order per map is path -> crf ->
    superpixel vote -> sieve -> scores.  With weight "confidence" the path is asked for its confidence map whether score_maps is
    given or not (the CRF-refined one with crf, the calibrated one under a temperature; the temperature rules stay as they are), and
    without score_maps nothing else of the score maps appears.  Score maps and Calibration lines stay those of the UNVOTED labels, as
    with the sieve.  Every rank votes the whole map itself and gets the same bits.  One line `---- Iter N -- Test Map M: Superpixel
    size= s compactness= m iters= i weight= ... Regions= r Changed Pixels= p` follows the map's other lines (before the Sieve line),
    and one for all maps with the counts summed.  Returns (all-maps confusion matrix, label maps, extra) with extra["superpixel"] =
    {"params": the SuperpixelParams, "per_map": [superpixel_vote's info per map], "regions", "changed_pixels" (summed)}.  Without
    superpixel nothing changes."""
    from . import _lib
    comm = comm or NoComm()
    path = InferencePath(crop_size, crop_sizes, flavour, dense_tile, dense_tta, dense_scales, dense_se)
    path.check()
    crf = None if crf is None else P.check_crf(crf)
    beta = _check_temperature(temperature_beta, score_maps, crf)
    bdist = None if boundary_scores is None else P.check_boundary_distances(boundary_scores)
    sieve = None if sieve is None else P.check_sieve(sieve)
    spx = None if superpixel is None else P.check_superpixel(superpixel)
    oconn = None if object_scores is None else P.check_object_scores(object_scores)
    stol = None if surface_scores is None else P.check_surface_tolerances(surface_scores)
    cal_tail = "" if beta is None else " Temperature= " + "{:.6f}".format(1.0 / beta)
    kinds = None
    if score_maps is not None:
        kinds = P.check_score_kinds(score_maps)
        kinds = kinds if "confidence" in kinds else kinds + ("confidence",)
        all_hist = np.zeros((256, 2), dtype=np.int64)
        score_list, cal_list = [], []
    # the confidence-weighted vote needs the path's confidence map, as the calibration report does: asked for, not reported
    run_kinds = ("confidence",) if kinds is None and spx is not None and spx.weight == "confidence" else kinds
    K = net.plan.K
    if sieve is not None:
        P.sieve_thresholds(sieve, K)
        sieve_list = []
    if spx is not None:
        spx_list = []
    pool = pool or P.TilePool(testing_data, testing_labels, net.dev)
    all_cm = np.zeros((K, K), dtype=np.uint32)
    all_kappa = np.zeros(len(testing_data), dtype=np.float32)
    all_f1 = np.zeros(len(testing_data), dtype=np.float32)
    all_f1_per_class = np.zeros(K, dtype=np.float32)
    maps = []
    if bdist is not None:
        all_bhist = np.zeros((len(bdist) + 1, len(bdist) + 1, K, K), dtype=np.int64)
        boundary_list = []
    if oconn is not None:
        all_otable = np.zeros((K, 4, 32), dtype=np.int64)
        object_list = []
    if stol is not None:
        all_stable = np.zeros((2, K, MT.SURFACE_BINS + 2), dtype=np.int64)
        surface_list = []
    for k in range(len(testing_data)):
        pred, smaps = _run_path(path, net, pool, k, batch_size, mean_full, std_full, comm, run_kinds, beta, crf)
        h, w = pool.h[k], pool.w[k]
        voted = pred                                       # the labels the posterior voted for: what the score maps describe
        if spx is not None:
            pred, pinfo = superpixel_vote(net, pool, k, pred, spx, confidence=smaps["confidence"] if spx.weight == "confidence" else None)
            spx_list.append(pinfo)
        if sieve is not None:
            pred, sinfo = sieve_labels(pred, h, w, K, sieve, stream=net._stream())
            sieve_list.append(sinfo)
        conf = torch.zeros(K * K, dtype=torch.int32, device=net.dev)
        lab = pool.labels[int(pool.lab_off[k].item()):int(pool.lab_off[k].item()) + h * w]
        _lib.call("drs_confusion", lab.data_ptr(), pred.data_ptr(), None, h * w, K, ignore_label, conf.data_ptr(), net._stream())
        cm = conf.cpu().numpy().reshape(K, K).astype(np.uint32)
        all_cm += cm
        total, oa, na = MT.overall_and_normalized(cm)
        f1c, present = MT.f1_per_class(cm)
        f1_full = np.zeros(K, dtype=np.float32)
        f1_full[present] = f1c
        all_kappa[k], all_f1[k] = MT.cohen_kappa(cm), MT.f1_macro(cm)
        all_f1_per_class += f1_full
        maps.append(pred.cpu().numpy())
        if comm.rank == 0:
            print("---- Iter " + str(step) +
                  " -- Test Map " + str(testing_instances[k]) + ": Overall Accuracy= " + str(total) +
                  " Overall Accuracy= " + "{:.6f}".format(oa) +
                  " Normalized Accuracy= " + "{:.6f}".format(na) +
                  " F1 Score per class= " + np.array_str(f1_full).replace("\n", "") +
                  " F1 Score= " + "{:.4f}".format(all_f1[k]) +
                  " Kappa= " + "{:.4f}".format(all_kappa[k]) +
                  " Confusion Matrix= " + _cm_str(cm))
        if kinds is not None:
            hist = torch.zeros(512, dtype=torch.int64, device=net.dev)
            _lib.call("drs_reliability_histogram", lab.data_ptr(), voted.data_ptr(), smaps["confidence"].data_ptr(), h * w, K, ignore_label,
                      hist.data_ptr(), net._stream())
            hist = hist.cpu().numpy().reshape(256, 2)
            all_hist += hist
            score_list.append({kd: v.cpu().numpy() for kd, v in smaps.items()})
            cal_list.append(MT.calibration(hist))
            if comm.rank == 0:
                print("---- Iter " + str(step) + " -- Test Map " + str(testing_instances[k]) + ": " + _calibration_str(cal_list[-1]) + cal_tail)
        if bdist is not None:
            bhist = boundary_histogram(lab, pred, h, w, K, ignore_label, bdist, stream=net._stream()).cpu().numpy()
            all_bhist += bhist
            boundary_list.append(MT.boundary_scores(bhist, bdist))
            if comm.rank == 0:
                print("---- Iter " + str(step) + " -- Test Map " + str(testing_instances[k]) + ": " + _boundary_str(boundary_list[-1]))
        if spx is not None and comm.rank == 0:
            print("---- Iter " + str(step) + " -- Test Map " + str(testing_instances[k]) + ": " + _superpixel_str(spx, pinfo))
        if sieve is not None and comm.rank == 0:
            print("---- Iter " + str(step) + " -- Test Map " + str(testing_instances[k]) + ": " + _sieve_str(sieve, sinfo))
        if oconn is not None:
            otable = object_table(lab, pred, h, w, K, ignore_label, oconn).cpu().numpy()       # on the current stream: the net's
            all_otable += otable
            object_list.append(dict(MT.object_scores(otable), table=otable))
            if comm.rank == 0:
                print("---- Iter " + str(step) + " -- Test Map " + str(testing_instances[k]) + ": " + _objects_str(oconn, object_list[-1]))
        if stol is not None:
            stable = surface_histogram(lab, pred, h, w, K, ignore_label, stream=net._stream()).cpu().numpy()
            all_stable += stable
            surface_list.append(dict(MT.surface_scores(stable, stol), table=stable))
            if comm.rank == 0:
                print("---- Iter " + str(step) + " -- Test Map " + str(testing_instances[k]) + ": " + _surface_str(surface_list[-1]))
    total, oa, na = MT.overall_and_normalized(all_cm)
    if comm.rank == 0:
        print("---- Iter " + str(step) +
              " -- Test ALL MAPS: Overall Accuracy= " + str(total) +
              " Overall Accuracy= " + "{:.6f}".format(oa) +
              " Normalized Accuracy= " + "{:.6f}".format(na) +
              " F1 Score= " + np.array_str(all_f1).replace("\n", " ") +
              " Mean F1 Score= " + "{:.6f}".format(np.sum(all_f1) / float(len(testing_data))) +
              " F1 Score per class= " + np.array_str(all_f1_per_class / float(len(testing_data))).replace("\n", "") +
              " Kappa= " + np.array_str(all_kappa).replace("\n", " ") +
              " Mean Kappa Score= " + "{:.6f}".format(np.sum(all_kappa) / float(len(testing_data))) +
              " Confusion Matrix= " + _cm_str(all_cm))
    if kinds is not None:
        cal = MT.calibration(all_hist)
        cal["per_map"] = cal_list
        if comm.rank == 0:
            print("---- Iter " + str(step) + " -- Test ALL MAPS: " + _calibration_str(cal) + cal_tail)
        extra = {"scores": score_list, "reliability": all_hist, "calibration": cal}
        if beta is not None:
            extra["temperature_beta"] = beta
    if bdist is not None:
        bnd = MT.boundary_scores(all_bhist, bdist)
        bnd["per_map"] = boundary_list
        bnd["hist"] = all_bhist
        if comm.rank == 0:
            print("---- Iter " + str(step) + " -- Test ALL MAPS: " + _boundary_str(bnd))
        extra = dict(extra if kinds is not None else {}, boundary=bnd)
    if spx is not None:
        if comm.rank == 0:
            print("---- Iter " + str(step) + " -- Test ALL MAPS: " + _superpixel_str(spx, spx_list))
        sp = {"params": spx, "per_map": spx_list}
        for key in ("regions", "changed_pixels"):
            sp[key] = sum(i[key] for i in spx_list)
        extra = dict(extra if kinds is not None or bdist is not None else {}, superpixel=sp)
    if sieve is not None:
        if comm.rank == 0:
            print("---- Iter " + str(step) + " -- Test ALL MAPS: " + _sieve_str(sieve, sieve_list))
        sv = {"params": sieve, "per_map": sieve_list, "rounds": max([i["rounds"] for i in sieve_list] or [0])}
        for key in ("merged", "changed_pixels", "left_small"):
            sv[key] = sum(i[key] for i in sieve_list)
        for key in ("objects_before", "objects_after"):
            sv[key] = [sum(i[key][c] for i in sieve_list) for c in range(K)]
        extra = dict(extra if kinds is not None or bdist is not None or spx is not None else {}, sieve=sv)
    if oconn is not None:
        obj = dict(MT.object_scores(all_otable), connectivity=oconn, table=all_otable, per_map=object_list)
        if comm.rank == 0:
            print("---- Iter " + str(step) + " -- Test ALL MAPS: " + _objects_str(oconn, obj))
        extra = dict(extra if kinds is not None or bdist is not None or sieve is not None or spx is not None else {}, objects=obj)
    if stol is not None:
        srf = dict(MT.surface_scores(all_stable, stol), table=all_stable, per_map=surface_list)
        if comm.rank == 0:
            print("---- Iter " + str(step) + " -- Test ALL MAPS: " + _surface_str(srf))
        extra = dict(extra if kinds is not None or bdist is not None or sieve is not None or spx is not None or oconn is not None else {},
                     surface=srf)
    if kinds is not None or bdist is not None or sieve is not None or spx is not None or oconn is not None or stol is not None:
        return all_cm, maps, extra
    return all_cm, maps


def generate_final_maps(net, testing_data, testing_instances, batch_size, mean_full, std_full, update_type,
                        distribution_type, values, dataset, output_path, patch_acc_loss=None, patch_occur=None, comm=None,
                        dense_tile=None, dense_tta=None, dense_scales=None, dense_se=None, score_maps=None, temperature_beta=None,
                        crf=None, sieve=None, superpixel=None, polygons=None):
    """isprs:1854-1957: best (or fixed) patch size, sliding-window label map per tile, written as the reference's colour TIFF
    (`top_mosaic_09cm_area<i>_class.tif` / `top_potsdam_<i>_label.tif`) and as class ids (`.npy`).  dense_tile (an int, 0 = the
    default side): the maps come from overlap-tile inference (predict_tile_dense; no patch size is chosen); files as before.  dense_tta
    ("flip", "d4" or a tuple of codes; with dense_tile only): its dihedral test-time augmentation (predict_tile_dense's tta).
    dense_scales (a list of factors; with dense_tile only): its multi-scale test-time augmentation (predict_tile_dense's scales).
    dense_se ("global"; with dense_tile only, nets with squeeze-and-excitation blocks): its whole-image gates (predict_tile_dense's se).
    score_maps (opt-in; a tuple of kinds from patches.SCORE_KINDS; any inference path): per-pixel score maps written
    beside each label file as `<stem>_<kind>.npy` (uint8 [h, w]) and an 8-bit grey `<stem>_<kind>.tif`, by rank 0 as the labels are;
    returns (label maps, [per map {kind: uint8 numpy [h, w]}]).  temperature_beta (opt-in; with score_maps only; an inverse
    temperature): the score files are of the calibrated probabilities; the label files do not change.
    crf (opt-in; any inference path; what patches.check_crf accepts): the written maps and score maps are those of the path's
    posterior refined by a local dense CRF against the image (refine_crf).  With crf a temperature_beta is accepted
    without score_maps: it scales the unary, so with a CRF it CAN change the label files.
    sieve (opt-in; any inference path; what patches.check_sieve accepts): the written and returned maps are sieved to a minimum
    mapping unit first (sieve_labels), the refined map with crf; the score files stay those of the unsieved labels.
    superpixel (opt-in; any inference path; what patches.check_superpixel accepts): the written and returned maps are voted inside the
    superpixels of each map's image first (superpixel_vote), after crf and before sieve; with weight "confidence"
    the path is asked for its confidence map whether score_maps is given or not.  The score files stay those of the unvoted labels.
    polygons (opt-in; any inference path; 4 or 8, patches.check_polygons): the map that is written -- after crf, superpixel and sieve
    -- is also written as polygons (the module's polygons(); vectors.write_geojson): rank 0 writes `<stem>.geojson`
    beside the label files, one Polygon feature per connected region of a class, in pixel-corner coordinates, y down, and prints one
    line `Final Map M: Polygons connectivity= c Polygons per class= [..] Holes= n Vertices= n` per map and one `Final ALL MAPS: ...`
    with the counts summed.  Only rank 0 traces, and only where an output path is given.  The return values do not change.  Without
    polygons nothing changes: no launch, no line, no file."""
    comm = comm or NoComm()
    path = InferencePath(dense_tile=dense_tile, dense_tta=dense_tta, dense_scales=dense_scales, dense_se=dense_se)
    path.check()
    crf = None if crf is None else P.check_crf(crf)
    beta = _check_temperature(temperature_beta, score_maps, crf)
    kinds = None if score_maps is None else P.check_score_kinds(score_maps)
    sieve = None if sieve is None else P.check_sieve(sieve)
    spx = None if superpixel is None else P.check_superpixel(superpixel)
    pconn = None if polygons is None else P.check_polygons(polygons)
    poly_list = []
    run_kinds = kinds                                      # the confidence-weighted vote needs the path's confidence map: asked for, not written
    if spx is not None and spx.weight == "confidence" and "confidence" not in (kinds or ()):
        run_kinds = (kinds or ()) + ("confidence",)
    if sieve is not None:
        P.sieve_thresholds(sieve, net.plan.K)
    score_list = []
    sized = distribution_type in ("multi_fixed", "uniform", "multinomial")
    if dense_tile is None:
        path = path._replace(crop_size=(select_best_patch_size(distribution_type, values, patch_acc_loss, patch_occur, update_type,
                                                               debug=comm.rank == 0) if sized else int(values[0])))
    pool = P.TilePool(testing_data, None, net.dev)
    maps = []
    for k in range(len(testing_data)):
        pred, smaps = _run_path(path, net, pool, k, batch_size, mean_full, std_full, comm, run_kinds, beta, crf)
        if spx is not None:
            pred, _ = superpixel_vote(net, pool, k, pred, spx, confidence=smaps["confidence"] if spx.weight == "confidence" else None)
        if sieve is not None:
            pred, _ = sieve_labels(pred, pool.h[k], pool.w[k], net.plan.K, sieve, stream=net._stream())
        maps.append(pred.cpu().numpy())
        if kinds is not None:
            score_list.append({kd: v.cpu().numpy() for kd, v in smaps.items() if kd in kinds})
        if comm.rank == 0 and output_path:
            # isprs:1950-1955: the colour map under the reference's file names (ISPRS palette, isprs:118-139), plus the class ids as .npy
            from . import datasets
            stem = ("top_mosaic_09cm_area" + str(testing_instances[k]) + "_class" if dataset == "vaihingen"
                    else "top_potsdam_" + str(testing_instances[k]) + "_label")
            datasets.create_prediction_map(output_path + stem + ".tif", maps[-1])
            np.save(output_path + stem + ".npy", maps[-1])
            if kinds is not None:
                from PIL import Image
                for kd, v in score_list[-1].items():
                    np.save(output_path + stem + "_" + kd + ".npy", v)
                    Image.fromarray(v).save(output_path + stem + "_" + kd + ".tif")
            if pconn is not None:
                from . import vectors
                # `polygons` is this function's argument here (checked into pconn above): the module's polygons() by its other name
                table, verts, pinfo = _trace_polygons(pred.reshape(-1), pool.h[k], pool.w[k], pconn, stream=net._stream())
                vectors.write_geojson(output_path + stem + ".geojson", table, verts, net.plan.K)
                poly_list.append(_polygons_info(table, pinfo, net.plan.K))
                print("Final Map " + str(testing_instances[k]) + ": " + _polygons_str(pconn, poly_list[-1]))
    if poly_list:
        print("Final ALL MAPS: " + _polygons_str(pconn, poly_list))
    if kinds is not None:
        return maps, score_list
    return maps
