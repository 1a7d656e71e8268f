/*
 * drs.h -- C ABI of libdrs_hip.so: the MI355X (gfx950) kernels of the dilated-CNN multi-size patch
 * training / sliding-window (and opt-in overlap-tile) inference path of keillernogueira/dynamic-rs-segmentation.
 *
 * The reference has no FFI of its own: its device boundary is three `sess.run` call shapes
 * (isprs_dilated_random.py:1750-1752 train, :1274-1275 infer, :1588 validate) behind which TensorFlow runs
 * the ops listed below.  Each entry point here replaces one of those TensorFlow ops (or one per-pixel numpy
 * loop next to them) and cites the reference line it stands in for.  The host-side mirror of the reference's
 * net builders and step loops (dynamic-rs-segmentation_amd/net.py, loops.py) binds exactly these symbols.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (any allocator; PyTorch-ROCm tensors in the host
 *     mirror); nothing is allocated, freed or synchronised inside the library;
 *   - `stream` is a hipStream_t (NULL = the default stream); calls only enqueue work;
 *   - every function returns 0 on success, DRS_ERR_ARG (1) for a rejected argument, DRS_ERR_HIP (2) for a
 *     launch failure; nothing throws across the boundary; not re-entrant on one set of buffers;
 *   - activations are channels-last (the reference's NHWC) with an explicit zero halo:
 *     a "view" (base, S, P, ld, coff) addresses a slab [B][S+2P][S+2P][ld] floats whose interior pixel
 *     (b, y, x), channel c of the slice lives at base[((b*(S+2P) + y+P)*(S+2P) + x+P)*ld + coff + c];
 *     P = 0 gives the reference's plain [B, S, S, C] tensor; filters are HWIO = [k][k][Cin][Cout] as in the
 *     reference (isprs:706);
 *   - B*S*S must be < 2^24, and every activation slab a convolution reads must stay below 4 GiB (2^30 floats): the kernels
 *     address with a wave-uniform 64-bit base plus 32-bit byte offsets;
 *   - ARGUMENT DOMAINS: every op-level entry point that launches a kernel states its domain ("Ranges, else DRS_ERR_ARG: ...") and
 *     rejects everything outside it before its first HIP call and before it reads a HOST-pointer argument; a pointer that the text
 *     does not call optional ("or NULL", "may be NULL") must not be NULL.  The bounds are what the kernels and their launches need:
 *     grid limits (65535 in y and z), fixed per-thread arrays, the alignment of 16-byte vector accesses (ld and coff multiples of 4
 *     floats; bases come from an allocator and are at least 16-byte aligned), 32-bit offsets, the halo against the padding, and a
 *     channel slice inside its row, 0 <= coff and coff + C <= ld ("a slice of C in (ld, coff)" below).  tests/test_abi_contract.py
 *     holds one violation per stated bound against the library.
 */
#ifndef DRS_H_
#define DRS_H_
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRS_OK 0
#define DRS_ERR_ARG 1
#define DRS_ERR_HIP 2

/* ---- tf.nn.atrous_conv2d / tf.nn.conv2d (SAME, stride 1) + tf.nn.bias_add  (isprs:710-713) -------------
 * out[p, coff_out + o] (=|+=) sum_{u,v,c} in[p + (u,v)*rate - pad_before, c] * w[u][v][c][o] + bias[o]
 * `in` is a haloed view with P >= max(pad_before, pad_after); cout a multiple of 32; cin a multiple of 32, or 8 / 16 for
 * conv1 (its 3..5 bands zero-padded by drs_crop_normalize, the filter by drs_filter_pad_cin -- see there for its size).
 * `out` is [B*S*S][ld_out].
 * stats_partial (or NULL; not together with accumulate): [ceil(B*S*S / drs_conv_mtile(cout))][cout][2], per M tile and
 * output channel (s, M2) = (sum of the tile's outputs, sum of their squared deviations from the TILE's mean): the first half
 * of train-mode batch norm (isprs:658-660), two-pass inside the tile as TensorFlow is two-pass over the batch;
 * drs_conv_stats_reduce combines the tiles.
 * The input-gradient pass is this same call on the haloed output gradient with the filter from
 * drs_filter_flip_transpose and pad_before := pad_after.
 * Ranges, else DRS_ERR_ARG (drs_conv_forward and drs_conv_forward_ws): in, w, out not NULL (bias, stats_partial, workspace may be);
 * B, S >= 1, B*S*S < 2^24; k, rate >= 1; cin in {8, 16} or a multiple of 32 (>= 32); cout a multiple of 32 (>= 32);
 * k*k*cin*cout < 2^31; 0 <= pad_before <= P and (k-1)*rate - pad_before <= P (the halo covers both pads);
 * B*(S+2P)^2*ld_in < 2^30; a slice of cin in (ld_in, coff_in), of cout in (ld_out, coff_out); cin < 32: ld_in and coff_in multiples
 * of 4; not accumulate together with stats_partial.  drs_conv_executed_ksteps: B, S, k, rate, cin >= 1, B*S*S < 2^24, cout a
 * multiple of 32 (>= 32), executed and total (HOST pointers) not NULL. */
int drs_conv_mtile(int cout);
/* drs_conv_forward_ws: the same with a caller-owned workspace (>= drs_conv_workspace_floats(cout) floats, 16-byte aligned, enables
 * every geometry; NULL, unaligned or too small for the cut the shape asks for: the plain launch of drs_conv_forward -- the cut, and with
 * it the association of the sums, follows from the shape and the device's CU count alone, never from the workspace size).  With it, launches of fewer than 4096 tiles run "stream-K": the K-steps of all
 * tiles are cut into equal ranges, one per workgroup and a whole number of workgroups per CU, the tiles that a cut crosses are
 * completed from partial sums in the workspace in a fixed order (bitwise reproducible; sums associate differently from
 * drs_conv_forward's).  This is the path of the per-rank batches of data parallelism (16 patches of 25..85 pixels a side). */
size_t drs_conv_workspace_floats(int cout);
/* 1 if drs_conv_forward_ws (full workspace) leaves out, for this shape, the filter-tap rows that meet only the zero halo for a whole
 * tile of 128 pixels (exact zeros: results do not change): plain launches of >= 4096 tiles, and any plain launch whose tiles are whole
 * image rows of whole patches (S = 32, 64, 128: those start their full tiles first, the skipping ones last); never a stream-K launch */
int drs_conv_halo_skip(int B, int S, int k, int rate, int pad_before, int cin, int cout);
/* K-steps (32 input channels of one filter tap, for one output tile) that drs_conv_forward_ws (full workspace, stats_partial NULL:
 * an input gradient or an inference forward; a launch that writes tile statistics keeps the tiles of 128 consecutive pixels) executes for this
 * shape, and the K-steps of the algorithm (every tap for every tile).  executed < total where taps that meet only the zero halo for a
 * whole tile are left out: tap rows of the tiles of 128 consecutive pixels (drs_conv_halo_skip), tap rows and columns where the
 * library groups the same pixel position of many images into a tile.  Returns DRS_OK or DRS_ERR_ARG. */
int drs_conv_executed_ksteps(int B, int S, int k, int rate, int pad_before, int cin, int cout, long long* executed, long long* total);
int drs_conv_forward_ws(const float* in, int B, int S, int P, int ld_in, int coff_in, const float* w, const float* bias,
                        int k, int rate, int pad_before, int cin, int cout, float* out, int ld_out, int coff_out,
                        int accumulate, float* stats_partial, float* workspace, size_t workspace_floats, void* stream);
int drs_conv_forward(const float* in, int B, int S, int P, int ld_in, int coff_in, const float* w, const float* bias,
                     int k, int rate, int pad_before, int cin, int cout, float* out, int ld_out, int coff_out,
                     int accumulate, float* stats_partial, void* stream);

/* ---- filter gradient of the same op (what tf.gradients emits for isprs:710-712) --------------------------
 * grad[u][v][c < cin_real][o] = sum_p x[p + (u,v)*rate - pad_before, c] * g[p, o];  x, g haloed views.
 * slab: workspace of drs_conv_wgrad_splits(...) * k*k*cin*cout floats (per-split partial sums, summed in
 * a fixed order -> bitwise reproducible).
 * Ranges, else DRS_ERR_ARG: x, g, slab, grad not NULL; B, S >= 1, B*S*S < 2^24; k, rate >= 1; cin in {8, 16} or a multiple of 32;
 * 1 <= cin_real <= cin; cout a multiple of 32 (>= 32); k*k*cin*cout < 2^31; 0 <= pad_before <= Px and (k-1)*rate - pad_before <= Px
 * (the halo of x covers both pads, as in the forward call: the kernels form the shifted pixel address in 32 bits and a short halo
 * wraps it); Pg >= 0, any width -- the halo of g is only skipped over, Px and Pg are independent; B*(S+2Px)^2*ld_x < 2^30 and
 * B*(S+2Pg)^2*ld_g < 2^30; a slice of cin in (ld_x, coff_x), of cout in (ld_g, coff_g); cin < 32: ld_x and coff_x multiples of 4. */
int drs_conv_wgrad_splits(int B, int S, int k, int cin, int cout);
int drs_conv_wgrad(const float* x, int B, int S, int Px, int ld_x, int coff_x, const float* g, int Pg, int ld_g,
                   int coff_g, int k, int rate, int pad_before, int cin, int cin_real, int cout, float* slab,
                   float* grad, void* stream);

/* wt[k-1-u][k-1-v][o][c] = w[u][v][c][o]: the filter of the input-gradient pass.
 * Ranges, else DRS_ERR_ARG: w, wt not NULL; k, cin, cout >= 1; k*k*cin*cout < 2^31 (the element index is an int). */
int drs_filter_flip_transpose(const float* w, float* wt, int k, int cin, int cout, void* stream);
/* wp[u][v][c < cin_pad][o] = c < cin ? w[u][v][c][o] : 0.  For cin_pad = 8 / 16 (conv1's 3..5 bands in an 8-channel slab: the
 * packed-tap form of drs_conv_forward, 32 / cin_pad taps to a K-step of 32 rows) the caller's `wp` holds
 * round_up(k*k*cin_pad, 32) * cout floats and the rows past the last tap must be ZERO (this call writes the first k*k*cin_pad rows).
 * Ranges, else DRS_ERR_ARG: w, wp not NULL; k, cin, cout >= 1; cin_pad >= cin; k*k*cin_pad*cout < 2^31. */
int drs_filter_pad_cin(const float* w, float* wp, int k, int cin, int cin_pad, int cout, void* stream);

/* ---- the same convolution in split-bf16 arithmetic (csrc/conv_split.hip) ---------------------------------------
 * An opt-in second arithmetic for isprs:710-713 and its gradients; the exact-fp32 entry points above stay the default.
 * Every fp32 operand x is carried as `nterms` bf16 terms, term s = round-to-nearest-even bf16 of what the earlier terms
 * left (x = t0 + t1 (+ t2) up to 2^-17 |x| / 2^-25 |x|), and a product is evaluated on the bf16 MFMA pipe as the
 * partial products t_i * u_j with i + j < nterms (3 products for 2 terms, 6 for 3), accumulated in fp32.
 * Term layout: interleaved at 32-channel granularity over the fp32 indexing e of the slab the terms mirror:
 * term s of element e sits at (e & ~31) * nterms + 32 * s + (e & 31), 2 bytes each, so views need ld and coff
 * multiples of 32.  Filter terms are K-contiguous rows interleaved the same way (see drs_filter_split).
 *   drs_split_terms    : n fp32 (n % 32 == 0) -> their terms (a whole slab, halo included).
 *   drs_filter_split   : HWIO filter -> wf = forward operand [cout][k*k*cin_pad] and, if wd != NULL, wd = input-gradient
 *                        operand [cin][k*k*cout] (taps reversed: what drs_filter_flip_transpose is to the fp32 path).
 *   drs_conv_forward_split : drs_conv_forward on terms (`in`, `w`); cout % 64 == 0.  The input-gradient pass is the same
 *                        call on the terms of the haloed output gradient with wd and pad_before := pad_after.
 *                        stats_partial rows hold drs_split_conv_mtile(cout) pixels.
 *   drs_conv_wgrad_split : drs_conv_wgrad on terms; slab = drs_conv_wgrad_split_splits(..., Pg, nterms) * k*k*cin*cout floats
 *                        (an upper bound that is monotone in B and S: a slab sized for (b_max, s_max) serves every smaller call).
 *                        With Pg > 0 pixels past the end read the gradient slab's first halo pixel (zeros).
 * Ranges, else DRS_ERR_ARG: every pointer but bias, stats_partial and wd not NULL; nterms 2 or 3.
 *   drs_split_terms    : n a multiple of 32 (n == 0 does nothing).
 *   drs_filter_split   : k, cin >= 1; cin_pad >= cin, a multiple of 32; cout a multiple of 32 (>= 32); with wd: cin a multiple of 32;
 *                        k*k*cin_pad*cout*nterms < 2^31.
 *   drs_conv_forward_split : B, S >= 1, B*S*S < 2^24; k, rate >= 1; cin a multiple of 32 (>= 32); cout a multiple of 64 (>= 64);
 *                        0 <= pad_before <= P and (k-1)*rate - pad_before <= P; a slice of cin in (ld_in, coff_in), both multiples of 32;
 *                        a slice of cout in (ld_out, coff_out); B*(S+2P)^2*ld_in*nterms < 2^31 and k*k*cin*cout*nterms < 2^31 (32-bit
 *                        byte offsets into the term images); not accumulate together with stats_partial.
 *   drs_conv_wgrad_split : B, S >= 1, B*S*S < 2^24; k, rate >= 1; cin a multiple of 32 (>= 32); 1 <= cin_real <= cin; cout a multiple
 *                        of 64 (>= 64); k*k*cin*cout < 2^31; 0 <= pad_before <= Px and (k-1)*rate - pad_before <= Px; Pg >= 0 (Pg == 0
 *                        runs the register-staged form: there is no halo pixel to fetch zeros from); a slice of cin in (ld_x, coff_x),
 *                        of cout in (ld_g, coff_g), all four multiples of 32; B*(S+2Px)^2*ld_x*nterms < 2^32 and
 *                        B*(S+2Pg)^2*ld_g*nterms < 2^31. */
int drs_split_conv_mtile(int cout);
int drs_split_terms(const float* src, size_t n, int nterms, unsigned short* terms, void* stream);
int drs_filter_split(const float* w, int k, int cin, int cin_pad, int cout, int nterms, unsigned short* wf,
                     unsigned short* wd, void* stream);
int drs_conv_forward_split(const unsigned short* in, int B, int S, int P, int ld_in, int coff_in, const unsigned short* w,
                           const float* bias, int k, int rate, int pad_before, int cin, int cout, float* out, int ld_out,
                           int coff_out, int accumulate, float* stats_partial, int nterms, void* stream);
int drs_conv_wgrad_split_splits(int B, int S, int k, int cin, int cout, int Pg, int nterms);
int drs_conv_wgrad_split(const unsigned short* x, int B, int S, int Px, int ld_x, int coff_x, const unsigned short* g,
                         int Pg, int ld_g, int coff_g, int k, int rate, int pad_before, int cin, int cin_real, int cout,
                         float* slab, float* grad, int nterms, void* stream);

/* ---- tf.contrib.layers.batch_norm(center=False, scale=False, eps=1e-3, decay=0.999)  (isprs:655-663) -----
 * drs_stats_reduce : partial[nrows][C][2] (fp32) plain column sums -> sums[C][2] (fp64), fixed order (the backward
 *                    pass's (sum g, sum g*xhat) slabs); scratch is unused (kept in the signature).
 * drs_conv_stats_reduce : the statistics slab of drs_conv_forward (M = B*S*S pixels, mtile = drs_conv_mtile(cout) or
 *                    drs_split_conv_mtile(cout)) -> sums[C][2] = (sum z, sum z^2) in fp64 by Chan's combination
 *                    sum z^2 = sum_tiles (M2 + s^2 / n_tile): no cancellation in fp32 whatever |mean| / std is.
 *                    Under data parallelism the caller all-reduces `sums` between this call and drs_bn_finish
 *                    (sync batch norm over the global batch).
 * drs_conv_stats_finish : drs_conv_stats_reduce + drs_bn_finish in ONE launch (single rank); sums may be NULL.
 * drs_bn_finish    : sums, count -> mean_rstd[C][2] = (mean, 1/sqrt(biased var + eps)); if moving_* != NULL,
 *                    moving -= (moving - batch) * (1 - decay) with the Bessel-corrected variance when bessel.
 * drs_bn_eval_coeffs: is_training=False branch: mean_rstd from the moving statistics.
 * Ranges, else DRS_ERR_ARG: partial, mean_rstd / means (where the call writes them) not NULL, sums not NULL where the text does not
 * say it may be; moving_mean and moving_var both NULL or both given; nrows, C, M, mtile >= 1; count finite and >= 1; decay finite in
 * [0, 1].  drs_rows_reduce_f32: nrows, ncols >= 1; drs_sum_f64, drs_scale_f64: n >= 1. */
int drs_colsum_scratch_doubles(int ncols);
int drs_stats_reduce(const float* partial, int nrows, int C, double* sums, double* scratch, void* stream);
/* drs_stats_reduce that also leaves means[C][2] = (float)(sums / count): what drs_bn_backward_apply_means takes (single rank: the
 * sums need no all-reduce between the two); sums may be NULL */
int drs_stats_reduce_means(const float* partial, int nrows, int C, double count, double* sums, float* means, void* stream);
int drs_conv_stats_reduce(const float* partial, int M, int mtile, int C, double* sums, double* scratch, void* stream);
int drs_conv_stats_finish(const float* partial, int M, int mtile, int C, double count, float* mean_rstd, float* moving_mean,
                          float* moving_var, double decay, int bessel, double* sums, void* stream);
int drs_bn_finish(const double* sums, double count, int C, float* mean_rstd, float* moving_mean, float* moving_var,
                  double decay, int bessel, void* stream);
int drs_bn_eval_coeffs(const float* moving_mean, const float* moving_var, int C, float* mean_rstd, void* stream);

/* ---- normalise + tf.nn.relu | tf.maximum(0.1x, x) + tf.nn.max_pool(3x3, stride 1, SAME) ------------------
 * (isprs:715-721, 620-621, 745-746, 1001).  z: [B*S*S][C] raw conv output; alpha = 0 (ReLU) or 0.1;
 * pool: bit 0 = apply the 3x3 max-pool; bit 1 = the halo of `out` is known to be zero already (a previous call on this slab with
 * the same B, S, P_out wrote it and nothing else has written the slab since) and need not be rewritten (pooling path only).
 * out: haloed view (the halo zeros are written here); argmax (pool only, may be NULL): [B*S*S][C] window
 * position 0..8 of the first maximum, which the backward pass routes gradients to (TF MaxPoolGrad).
 * Ranges, else DRS_ERR_ARG (the three forward calls): z, mean_rstd not NULL, out not NULL (drs_bn_act_pool_forward_terms: out or
 * terms); B, S >= 1, P_out >= 0, B*(S+2*P_out) <= 65535 (grid.y), B*S*S < 2^24; C a multiple of 4 (>= 4); alpha finite in [0, 1]
 * (max(alpha x, x) is the activation only there); a slice of C in (ld_out, coff_out), both multiples of 4 (16-byte stores), with
 * terms multiples of 32 and nterms 2 or 3.  drs_bn_finish_act_pool_forward also: sums not NULL, count finite >= 1, decay finite in
 * [0, 1], moving_mean and moving_var both or neither, pool bit 0 set, C <= 512. */
int drs_bn_act_pool_forward(const float* z, int B, int S, int C, const float* mean_rstd, float alpha, int pool,
                            float* out, int P_out, int ld_out, int coff_out, unsigned char* argmax, void* stream);
/* drs_bn_finish + drs_bn_act_pool_forward in one launch (pooled blocks with C <= 512): under data parallelism the batch-norm sums
 * come back from an all-reduce, and the kernel that normalises works (mean, rstd) out of them itself (drs_bn_finish's arithmetic, the
 * same bits), leaves them in mean_rstd for the backward pass and updates the moving averages (isprs:655-663).  pool must have bit 0 set. */
int drs_bn_finish_act_pool_forward(const double* sums, double count, float* mean_rstd, float* moving_mean, float* moving_var, double decay,
                                   int bessel_moving_var, const float* z, int B, int S, int C, float alpha, int pool, float* out, int P_out,
                                   int ld_out, int coff_out, unsigned char* argmax, void* stream);
/* the same, also (out != NULL) or only (out == NULL) writing the split-bf16 terms of the output slab (layout above) */
int drs_bn_act_pool_forward_terms(const float* z, int B, int S, int C, const float* mean_rstd, float alpha, int pool,
                                  float* out, int P_out, int ld_out, int coff_out, unsigned char* argmax,
                                  unsigned short* terms, int nterms, void* stream);

/* ---- backward of the block above ----------------------------------------------------------------------
 * reduce: ga [B*S*S][ld_ga]+coff_ga = gradient wrt the block output -> gxhat [B*S*S][C] (gradient wrt the
 *         normalised activation) and partial[drs_bn_backward_rows(B,S,C,pool)][C][2] = (sum g, sum g*xhat);
 * apply : gz = rstd * (gxhat - sum_g/count - xhat * sum_gx/count) into a haloed view (halo zeroed).
 * Ranges, else DRS_ERR_ARG: every pointer not NULL (argmax only with pool; gz may be NULL in drs_bn_backward_apply_terms); B, S >= 1,
 * B*S*S < 2^24; C a multiple of 4, 4 <= C <= 1024; reduce: B*S <= 65535, alpha finite in [0, 1], a slice of C in (ld_ga, coff_ga),
 * both multiples of 4 (16-byte loads); apply: P_out >= 0, B*(S+2*P_out) <= 65535, count finite >= 1, a slice of C in
 * (ld_out, coff_out), both multiples of 4, with terms multiples of 32 and nterms 2 or 3. */
int drs_bn_backward_rows(int B, int S, int C, int pool);
int drs_bn_backward_reduce(const float* ga, int ld_ga, int coff_ga, const float* z, const unsigned char* argmax, int B,
                           int S, int C, const float* mean_rstd, float alpha, int pool, float* gxhat, float* partial,
                           void* stream);
int drs_bn_backward_apply(const float* gxhat, const float* z, int B, int S, int C, const float* mean_rstd,
                          const double* sums, double count, float* gz, int P_out, int ld_out, int coff_out,
                          void* stream);
/* drs_bn_backward_apply with the two means as fp32 from drs_stats_reduce_means (the same bits; no fp64 division per workgroup) */
int drs_bn_backward_apply_means(const float* gxhat, const float* z, int B, int S, int C, const float* mean_rstd,
                                const float* means, float* gz, int P_out, int ld_out, int coff_out, void* stream);
/* the same, also (gz != NULL) or only (gz == NULL) writing the split-bf16 terms of the haloed gradient */
int drs_bn_backward_apply_terms(const float* gxhat, const float* z, int B, int S, int C, const float* mean_rstd,
                                const double* sums, double count, float* gz, int P_out, int ld_out, int coff_out,
                                unsigned short* terms, int nterms, void* stream);

/* ---- tf.nn.avg_pool(k x k, stride 1, SAME) of the `_avgpool` variant (isprs:753-758, 818-854) ------------------
 * forward: in [B*S*S][C] -> interior of a haloed view (halo zeroed), divisor = pixels of the window inside the image;
 * backward: gout [B*S*S][ld_g]+coff_g -> gin [B*S*S][C].  k odd.
 * Ranges, else DRS_ERR_ARG: pointers not NULL; k odd, >= 1; B, S >= 1, P_out >= 0, B*(S+2*P_out) <= 65535 (backward: B*S), B*S*S < 2^24;
 * C a multiple of 4 (>= 4); a slice of C in (ld_out, coff_out) / (ld_g, coff_g), both multiples of 4. */
int drs_avg_pool_forward(const float* in, int B, int S, int C, int k, float* out, int P_out, int ld_out, int coff_out,
                         void* stream);
int drs_avg_pool_backward(const float* gout, int ld_g, int coff_g, int B, int S, int C, int k, float* gin, void* stream);

/* ---- _squeeze_excitation_layer of the `_SE` variant (isprs:682-697, _fc_layer :666-679) -------------------------
 * forward : act [B*S*S][C] (activated block output) -> s = spatial mean, e1 = relu(s w1 + b1) [B][R], e2 = sigmoid(e1 w2 + b2)
 *           [B][C] (all three kept for the backward pass), out view = act * e2 (halo zeroed);  w1 [C][R], w2 [R][C].
 * backward: gy (gradient wrt the scaled output) -> gact [B*S*S][C] and the four parameter gradients (sums over this rank's
 *           images, fixed order); scratch: B*(3*C + R) floats.
 * Ranges, else DRS_ERR_ARG (drs_se_forward, drs_se_backward, drs_se_scale_const): pointers not NULL; B, S >= 1, P_out >= 0,
 * B*(S+2*P_out) <= 65535 (backward: B*S), B*S*S < 2^24; C a multiple of 4 (>= 4); R >= 1; C + R <= 16384 (the excite kernels keep
 * both vectors in LDS); a slice of C in (ld_out, coff_out) / (ld_g, coff_g), both multiples of 4. */
int drs_se_forward(const float* act, int B, int S, int C, int R, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* s, float* e1, float* e2, float* out, int P_out, int ld_out, int coff_out, void* stream);
int drs_se_backward(const float* gy, int ld_g, int coff_g, const float* act, const float* s, const float* e1, const float* e2,
                    const float* w1, const float* w2, int B, int S, int C, int R, float* gact, float* dw1, float* db1, float* dw2,
                    float* db2, float* scratch, void* stream);
/* the same layer gated by the mean over a whole IMAGE that is forwarded in tiles (overlap-tile inference with se="global", DESIGN.md
 * 8a.3): the gate is then one constant vector per image, made in three steps.
 * drs_se_core_sums : act [n*T*T][C] (the activated block output of n tiles of side T) and boxes [n][6] = (y0, x0, cy0, cy1, cx0, cx1)
 *           (device data, drs_tile_place's layout): sums[c] += sum of act over every tile's core box (cores partition the image, so
 *           a whole plan counts every pixel once).  fp32 loads accumulated in fp64 in a fixed order, no atomics; launches on one
 *           stream accumulate in stream order.  A core that does not lie inside its tile adds nothing.  The caller zeroes sums when
 *           a sweep begins.  scratch: drs_se_core_sums_scratch_doubles(C) doubles.  n * T * T < 2^31.
 * drs_se_gate      : sums [C] over `count` pixels -> s = (float)(sums / count) (fp64 division, one rounding), e1 [R], e2 [C] by
 *           drs_se_forward's excite arithmetic for one image.
 * drs_se_scale_const: out view = act * e2[c] with ONE gate vector e2 [C] for the whole batch (halo zeroed).
 * Ranges, else DRS_ERR_ARG: pointers not NULL.  drs_se_core_sums: C >= 1, 1 <= T <= 65535, 1 <= n <= 65535, n*T*T < 2^31.
 * drs_se_gate: C, R >= 1, C + R <= 16384, count finite and > 0. */
int drs_se_core_sums_scratch_doubles(int C);
int drs_se_core_sums(const float* act, int C, int T, const int* boxes, int n, double* sums, double* scratch, void* stream);
int drs_se_gate(const double* sums, double count, int C, int R, const float* w1, const float* b1, const float* w2, const float* b2,
                float* s, float* e1, float* e2, void* stream);
int drs_se_scale_const(const float* act, int B, int S, int C, const float* e2, float* out, int P_out, int ld_out, int coff_out,
                       void* stream);

/* ---- 1x1 classifier + sparse softmax cross-entropy + tf.argmax (+ their gradients) ----------------------
 * (isprs:1024-1031, 1089-1099, 1690; masked loss: contest_dilated_random.py:881-901; confusion matrix:
 * calc_accuracy_by_crop isprs:510-531).  feat: haloed view with C channels (multiple of 64, <= 448);
 * w [C][K], K <= 8.  labels == NULL -> inference (logits / pred only).  inv_n = 1 / number of pixels the
 * loss averages over (all ranks).  Per-workgroup slabs (rows = drs_classifier_rows(B,S)):
 * dw_partial [rows][C][K], db_partial [rows][K], loss_partial [rows] (sum of per-pixel CE, fp64).
 * conf: [K][K] counters, ADDED to (integer atomics), rows = label, cols = prediction, gated by acc_mask.
 * Ranges, else DRS_ERR_ARG (the three classifier calls): feat, w, bias not NULL; with labels: loss_partial; with gfeat: labels,
 * dw_partial, db_partial; B, S >= 1, P >= 0, B*S*S < 2^24, B*(S+2P)^2*ld < 2^30; C a multiple of 64, 64..448; K 1..8; inv_n finite
 * and >= 0; a slice of C in (ld, coff) and, with gfeat, in (ld_g, coff_g), all multiples of 4 (16-byte accesses). */
int drs_classifier_rows(int B, int S);
int drs_classifier_loss(const float* feat, int B, int S, int P, int ld, int coff, int C, int K, const float* w,
                        const float* bias, const unsigned char* labels, const unsigned char* loss_mask,
                        const unsigned char* acc_mask, float inv_n, float* logits, unsigned char* pred, float* gfeat,
                        int ld_g, int coff_g, float* dw_partial, float* db_partial, double* loss_partial,
                        unsigned int* conf, void* stream);
/* The same with per-class weights (opt-in).  class_weights: HOST pointer to K finite, non-negative floats wc (copied
 * into the kernel arguments: no device buffer, no extra load), or NULL.  With weights the data term of the loss is
 *     L = inv_n * sum over the pixels p in the loss of wc[y_p] * CE_p
 * ("in the loss" as above: loss_mask set when given, y_p < K) and the logit gradient is wc[y_p] * (softmax_k - [k == y_p]) * inv_n:
 * gfeat, dw_partial, db_partial and loss_partial (sum of wc[y] * CE, fp64) follow from it; logits, pred and conf are not weighted.
 * The normaliser stays inv_n -- NOT 1 / sum wc[y_p], PyTorch's `weight=` convention: inv_n is known before the launch, so there is
 * no data-dependent pre-pass and no extra collective under data parallelism, and with "balanced" weights (sum_k f_k wc_k = 1 over
 * the class frequencies f) the expected scale of L is that of the unweighted loss.
 * NULL, or all K weights exactly 1.0f, or labels == NULL: the kernels of drs_classifier_loss, which do not multiply at all -- every
 * output bit for bit.  A negative or non-finite weight: DRS_ERR_ARG (K <= 8 as above). */
int drs_classifier_loss_weighted(const float* feat, int B, int S, int P, int ld, int coff, int C, int K, const float* w,
                                 const float* bias, const unsigned char* labels, const unsigned char* loss_mask,
                                 const unsigned char* acc_mask, float inv_n, const float* class_weights, float* logits,
                                 unsigned char* pred, float* gfeat, int ld_g, int coff_g, float* dw_partial, float* db_partial,
                                 double* loss_partial, unsigned int* conf, void* stream);
/* The same with the focal modulation (opt-in; Lin et al., "Focal loss for dense object detection").  focal_gamma is
 * the focusing parameter: 0, or finite in (0, 8]; anything else is DRS_ERR_ARG.  With wc the class weights (ones when class_weights
 * is NULL), P = softmax(logits_p) in the max-subtracted form (ex_k = exp(logit_k - max), se = sum_k ex_k), for a pixel in the loss:
 *     p_t = P[y]          q = 1 - p_t, formed as (sum over k != y, ascending, of ex_k) / se -- never as 1 - p_t, which cancels
 *     CE  = -log p_t      m = q^gamma, 0 at q == 0
 *     L   = inv_n * sum over the pixels in the loss of wc[y] * m * CE                      (the alpha-balanced focal loss)
 *     f   = m * (1 + gamma * p_t * r),  r = CE / q, taken as its limit 1 as q -> 0         (= q^g + g p_t q^(g-1) CE, no inf * 0)
 *     d L / d logit_k = wc[y] * f * (P_k - [k == y]) * inv_n
 * gfeat, dw_partial, db_partial follow from that gradient as in drs_classifier_loss; loss_partial is the fp64 sum of wc[y] * m * CE.
 * logits, pred and conf are not modulated.  inv_n stays the normaliser it is (not 1 / sum of modulators): no pre-pass, no collective.
 * focal_gamma == 0 (or labels == NULL) is NOT a focal launch: it is drs_classifier_loss_weighted, every output bit for bit.  With
 * focal_gamma > 0 the focal instantiations run and multiply wc[y] in even when it is one. */
int drs_classifier_loss_focal(const float* feat, int B, int S, int P, int ld, int coff, int C, int K, const float* w,
                              const float* bias, const unsigned char* labels, const unsigned char* loss_mask,
                              const unsigned char* acc_mask, float inv_n, const float* class_weights, float focal_gamma,
                              float* logits, unsigned char* pred, float* gfeat, int ld_g, int coff_g, float* dw_partial,
                              float* db_partial, double* loss_partial, unsigned int* conf, void* stream);
/* Ranges, else DRS_ERR_ARG (drs_label_histogram, drs_reliability_histogram): pointers not NULL; K 1..8; 1 <= n < 2^40.
 * per-class pixel counts of n label bytes (the class-weight recipes): counts[k] += #{i : labels[i] == k}, k < K <= 8, leaving out
 * labels equal to void_label (-1: none) or >= K; counts = K 64-bit counters on the device, ADDED to (integer atomics: exact and
 * order-independent), so the maps of a pool accumulate over several calls.  n < 2^40. */
int drs_label_histogram(const unsigned char* labels, size_t n, int K, int void_label, unsigned long long* counts, void* stream);
/* reliability table of a prediction (the calibration report, metrics.calibration): for every i < n with truth[i] != ignore_label
 * and truth[i] < K: hist[confidence[i]][0] += 1 and hist[confidence[i]][1] += (pred[i] == truth[i]).  hist = [256][2] 64-bit
 * counters on the device, ADDED to (integer atomics: exact and order-independent), so the maps of a split accumulate.  A prediction
 * >= K counts as wrong (drs_confusion leaves such a pixel out; a finalised map holds none).  K <= 8, n < 2^40. */
int drs_reliability_histogram(const unsigned char* truth, const unsigned char* pred, const unsigned char* confidence, size_t n, int K,
                              int ignore_label, unsigned long long* hist, void* stream);
/* temperature scaling (opt-in; Guo et al., On calibration of modern neural networks): the sufficient statistics of
 * the fit of ONE scalar, the inverse temperature beta = 1 / T, on labelled maps.  beta is finite and 1/64 <= beta <= 64; anything else
 * is DRS_ERR_ARG.  Per pixel i: oc = occur[i] ? occur[i] : 1, s_k = sums[i][k] (the accumulators handed to drs_stitch_finalize*).
 *   score vector u (fp64)   sums_are_prob == 0: u_k = (double)s_k / (double)oc
 *                           sums_are_prob != 0: q_k = s_k / (float)oc in fp32 (as drs_stitch_finalize_scores forms it), then
 *                                               u_k = log((double)max(q_k, FLT_MIN)): the log of the mean probability, which is the
 *                                               usual extension of temperature scaling to an ensemble
 *   calibrated p(beta)      softmax(beta u), max-subtracted
 *   counted pixels          occur[i] > 0, truth[i] != ignore_label and truth[i] < K (those drs_confusion counts, less the uncovered)
 * With mu = sum_k p_k u_k, y = truth[i], m = max_k beta u_k, summed over the counted pixels in fp64:
 *   out[0] += N   the count (exact below 2^53)
 *   out[1] += L = sum [ log sum_k exp(beta u_k - m) + m - beta u_y ]      the negative log-likelihood; convex in beta
 *   out[2] += G = sum (mu - u_y)                                           dL/dbeta
 *   out[3] += H = sum sum_k p_k (u_k - mu)^2                               d2L/dbeta2 >= 0
 *   out[4] += A = sum |mu - u_y|                                           the scale G is judged against
 * out = 5 doubles on the device, ADDED to in stream order, so the maps of a split accumulate over several calls.  No float atomics:
 * per-workgroup rows of `scratch` (drs_temperature_scratch_doubles(n) doubles, device) are added in a fixed order by a second
 * launch, and the grid depends on n alone, so two runs give the same bits.  K <= 8, n < 2^40; n == 0 does nothing.
 * Ranges, else DRS_ERR_ARG: pointers not NULL; K 1..8; n < 2^40; beta as above. */
size_t drs_temperature_scratch_doubles(size_t n);
int drs_temperature_stats(const float* sums, const unsigned int* occur, const unsigned char* truth, size_t n, int K, int sums_are_prob,
                          int ignore_label, double beta, double* scratch, double* out /* [5] = N, L, G, H, A: ADDED to */, void* stream);

/* fixed-order column sums (scratch: drs_colsum_scratch_doubles(ncols) doubles) / scalar sums used on the slabs above */
int drs_rows_reduce_f32(const float* in, int nrows, int ncols, float* out, double* scratch, void* stream);
int drs_sum_f64(const double* in, int n, double* out, void* stream);
int drs_scale_f64(double* x, int n, double s, void* stream);      /* x[i] *= s (the 1/N of the mean cross-entropy) */
/* tf.nn.l2_loss over the kernels (isprs:646-651): out[0] = 0.5 * sum w^2; scratch = 256 doubles.
 * Ranges, else DRS_ERR_ARG: pointers not NULL; 1 <= n < 2^40. */
int drs_l2_loss(const float* w, size_t n, double* scratch, double* out, void* stream);

/* ---- tf.train.MomentumOptimizer(momentum).minimize  (isprs:1685-1687) -----------------------------------
 * g = grad*grad_scale (+ weight_decay*w for the first n_decay entries = the kernels; biases are not decayed,
 * isprs:640-652); accum = momentum*accum + g; w -= lr*accum.
 * Ranges, else DRS_ERR_ARG: pointers not NULL; 1 <= n < 2^40; n_decay <= n. */
int drs_momentum_update(float* w, const float* grad, float* accum, size_t n, size_t n_decay, float lr,
                        float weight_decay, float momentum, float grad_scale, void* stream);

/* ---- calc_accuracy_by_crop / whole-map confusion loops  (isprs:510-531, 1290-1296) -----------------------
 * Ranges, else DRS_ERR_ARG: labels, pred, conf not NULL (mask may be); K 1..8; 1 <= n < 2^32 (conf holds 32-bit counters). */
int drs_confusion(const unsigned char* labels, const unsigned char* pred, const unsigned char* mask, size_t n, int K,
                  int ignore_label, unsigned int* conf, void* stream);

/* ---- dynamically_create_patches + normalize_images  (isprs:245-334, 74-81; tiler isprs:337-400) ----------
 * inst [B][4] = (map, row, col, flip) with the border shift-back already applied (isprs:260-269);
 * rot [B][6] = (m00 m01 m10 m11 off0 off1) of scipy.ndimage.rotate(order=0, reshape=False) when rot_on[b];
 * noise [B][S][S][C] (fp64, reference-exact) or NULL (device Philox N(0, 0.01) keyed by (seed, noise_index0 + b, element):
 * noise_index0 = index of this call's first patch in the global batch, so a sharded batch draws the same noise) when noise_on[b];
 * out: conv1 input slab [B][S+2P][S+2P][ld] (channels C..ld-1 and the halo are zeroed);
 * out_lab / out_mask [B][S][S] (uint8); out_mask is 0 where the rotation pulled in fill or the label equals
 * void_label (contest_dilated_random.py:235-239; -1 = none).  Normalisation touches channels 0,1,2 only.
 * mean3 / std3 are HOST pointers to 3 doubles each (copied into the kernel arguments).
 * quantize_f16: coffee_dilated_random.py:293 casts its training patches to float16 and :67-74 normalises them in that array:
 * value, value - mean and (value - mean) / std are each rounded to float16.  NumPy >= 2 evaluates float16-array (op) numpy-scalar in
 * the scalar's type: 1 = mean / std are float32 scalars (what coffee's compute_image_mean yields from its float32 patches, :78-79):
 * float32 arithmetic; 2 = float64 scalars (e.g. statistics read from a float64 .npy): float64 arithmetic.  (NumPy 1.x cast the
 * scalar to float16 first: not reproduced.)
 * Ranges, else DRS_ERR_ARG (drs_crop_normalize and drs_crop_normalize_scaled): tiles, labels, tile_off, lab_off, tile_h, tile_w, inst,
 * out, mean3, std3 (and geo) not NULL; rot, rot_on, noise, noise_on, out_lab, out_mask may be; C 1..8; ld >= C, a multiple of 4
 * (16-byte stores); B, S >= 1, P >= 0, B*(S+2P) <= 65535 (grid.y); noise_index0 >= 0; quantize_f16 0..2; n_maps >= 1. */
int drs_crop_normalize(const void* tiles, int tiles_are_f64, const unsigned char* labels, const long long* tile_off,
                       const long long* lab_off, const int* tile_h, const int* tile_w, int C, const int* inst,
                       const double* rot, const unsigned char* rot_on, const double* noise,
                       const unsigned char* noise_on, unsigned long long seed, int noise_index0, const double* mean3,
                       const double* std3,
                       int B, int S, int P, int ld, float* out, unsigned char* out_lab, unsigned char* out_mask,
                       int void_label, int quantize_f16, void* stream);
/* scale-jitter augmentation of training, fused into the crop (opt-in).  NORMATIVE: this text, the numpy statement
 * tests/scale_jitter_ref.py and the kernel say the same thing in the same operation order.
 * Patch b of side S has a scale s_b: it is the S x S image whose pixel centres sample the source map X (h x w) over a footprint of
 * side S / s_b around a centre (cy, cx) given in continuous pixel-edge coordinates (pixel i covers [i, i + 1], its centre is
 * i + 0.5).  geo [B][3] (fp64, device data) = (step, cy, cx) with step = 1 / s_b computed by the host in fp64.  Per axis -- map
 * length n, centre c, patch pixel index p in [0, S) -- every product and sum rounded on its own, in fp64:
 *     t = (p + 0.5) - 0.5 S,   u = c + t step                        the position of the pixel's centre
 *     valid on the axis iff 0 <= u <= n;  a pixel is valid iff both axes are
 *     src = min(max(u - 0.5, 0), n - 1),  i0 = floor(src),  i1 = min(i0 + 1, n - 1),  l = src - i0
 * and the value is D's expression (drs_crop_resampled below), (1-ly)((1-lx) v00 + lx v01) + ly((1-lx) v10 + lx v11), in fp64 on
 * every channel.  The label is that of the source pixel that contains the centre, X_lab[min(floor(u_y), h-1)][min(floor(u_x), w-1)].
 * An invalid pixel is filled as the rotation fills: value 0, label 0, mask 0.
 * The centre is the host's (patches.scale_geometry): with r the patch's row (column) after the border shift-back for side S
 * (isprs:260-269), c = r + S / 2; then, with a = S / (2 s_b): c = min(max(c, a), n - a) if 2 a <= n (a footprint that fits in the map
 * lies inside it), else c = n / 2 (the map is smaller than the footprint: the overhang is invalid and masked).
 * Everything else acts on this resampled patch as it acts on drs_crop_normalize's plain crop, in that order: the order-0 rotation
 * picks a patch pixel (si, sj), and it is that pixel that is resampled (p = si on the row axis, sj on the column axis); a rotated-in
 * pixel is invalid; the noise is added after the interpolation and indexed before the flip, from the host array or from Philox keyed
 * by the global patch index; quantize_f16 (the fp64 value rounded to float32, as coffee's patches are float32, then to float16) and
 * the normalisation of bands 0..2 follow; one rounding to fp32 on the store; out_mask = valid && label != void_label.
 * At s_b = 1 the weights are exactly (1, 0) and slab, labels and mask are drs_crop_normalize's bit for bit (values other than -0.0).
 *
 * drs_crop_normalize_scaled: drs_crop_normalize's arguments plus geo, and n_maps (the number of maps in the pool), which the
 * device-side check of geo needs.  inst [B][4] = (map, row, col, flip): row / col are not read (the centre is in geo).  geo and inst are
 * checked on the device, as drs_crop_resampled checks inst: a step that is not finite and positive, a centre that is not finite, or a
 * map index outside [0, n_maps), leaves that patch's slab all zeros (no noise), its labels 0 and its mask 0.  Every source index is
 * clamped into its map, so no finite geo reads outside the pool. */
int drs_crop_normalize_scaled(const void* tiles, int tiles_are_f64, const unsigned char* labels, const long long* tile_off,
                              const long long* lab_off, const int* tile_h, const int* tile_w, int n_maps, int C, const int* inst,
                              const double* geo, const double* rot, const unsigned char* rot_on, const double* noise,
                              const unsigned char* noise_on, unsigned long long seed, int noise_index0, const double* mean3,
                              const double* std3, int B, int S, int P, int ld, float* out, unsigned char* out_lab,
                              unsigned char* out_mask, int void_label, int quantize_f16, void* stream);

/* ---- overlap-add of window logits and arg-max of the average  (isprs:1261-1284, 1925-1949) ---------------
 * windows [first_window, first_window + n_windows) of the row-major window grid at `stride` (last row/col
 * shifted back to the border) are added, in that order, into prob [h][w][K] / occur [h][w].
 * THE STRIDE LIMIT: a coordinate may lie under at most 5 regular windows per axis, plus the shifted-back one -- the kernel lists a
 * pixel's windows in fixed arrays of 6 -- so ceil(S / stride) <= 5.  The reference's stride is floor(S / 2) (isprs:1243): 2 or 3.
 * Ranges, else DRS_ERR_ARG: pointers not NULL; K 1..8; h, w >= 1; 1 <= S <= min(h, w); stride >= 1 and (S + stride - 1) / stride <= 5;
 * first_window >= 0, n_windows >= 1, first_window + n_windows <= n_h * n_w (the window grid; n_h * n_w < 2^31); the image rows a call
 * touches <= 65535 (grid.y).  drs_stitch_finalize, drs_softmax_accumulate (below): pointers not NULL, K 1..8, h, w >= 1. */
int drs_stitch_accumulate(float* prob, unsigned int* occur, const float* logits, int h, int w, int K, int S, int stride,
                          int first_window, int n_windows, void* stream);
int drs_stitch_finalize(const float* prob, const unsigned int* occur, int h, int w, int K, unsigned char* out,
                        void* stream);
/* overlap-tile inference (opt-in, beside the reference's windows): n tiles of side T, each with its core box, from the
 * device array boxes [n][6] = (y0, x0, cy0, cy1, cx0, cx1) in image coordinates (tile origin, half-open core rows / columns).  For every
 * core pixel (y, x) the K logits logits[i][y - y0][x - x0][:] (a [n][T][T][K] block, as drs_forward writes it) are COPIED into
 * prob[y][x][:] and occur[y][x] += 1.  Labels: drs_stitch_finalize (occur = 1: an exact arg-max, first maximum).  K <= 8,
 * T <= min(h, w); the boxes are device data, checked on the device: a box outside the image or outside its tile places nothing (the
 * coverage count occur, 1 everywhere after a whole plan, shows the gap).  The tile plan itself is the host's.
 * Ranges, else DRS_ERR_ARG (drs_tile_place and drs_tile_place_dihedral): pointers not NULL; K 1..8; 1 <= T <= min(h, w), T <= 65535;
 * 1 <= n <= 65535 (grid.y, grid.z); g 0..7. */
int drs_tile_place(float* prob, unsigned int* occur, const float* logits, int h, int w, int K, int T, const int* boxes, int n,
                   void* stream);
/* dihedral test-time augmentation of overlap-tile inference (opt-in).  A transform code g in 0..7 is one of the 8
 * symmetries of the square (the group D4): bit 0 = fx (flip columns), bit 1 = fy (flip rows), bit 2 = t (transpose).  For a T x T
 * tile X the transformed tile is Y[i][j] = X[sigma_g(i, j)] with
 *     (i', j') = (fy ? T-1-i : i, fx ? T-1-j : j),   sigma_g(i, j) = t ? (j', i') : (i', j')      (flip, then transpose)
 * and logits L of Y go back onto X's grid through sigma_g^-1(a, b): transpose first, then flip.  sigma_g != sigma_g^-1 exactly for
 * g = 5 and g = 6 (the two quarter-turns).  drs_crop_normalize's flip codes are g = 2 (flip 1, flipud) and g = 1 (flip 2, fliplr).
 *
 * drs_crop_dihedral: conv1's input slab out [B][T+2P][T+2P][ld] of the g-transformed T x T tiles inst [B][3] = (map, row, col)
 * (device data), normalised as drs_crop_normalize normalises (fp64 until one rounding to fp32 on the store, bands 0..2 only; mean3 /
 * std3 are HOST pointers), with no augmentation, labels or mask; halo and channels C..ld-1 are zero.  A tile that does not lie
 * inside its map, or a map index outside [0, n_maps), is caught on the device: that patch's slab is all zeros.  g = 0 is
 * drs_crop_normalize with flip 0 and no augmentation, bit for bit.
 * drs_tile_place_dihedral: boxes as drs_tile_place (same device-side checks); for every core pixel (y, x) at tile-local
 * (a, b) = (y - y0, x - x0), softmax_k(logits[i][sigma_g^-1(a, b)][:]) (max-subtracted, fp32, classes summed in order) is ADDED
 * into acc[y][x][:] and occur[y][x] += 1.  K <= 8.  The cores of one call must be disjoint (plain read-modify-write of acc).
 * Ranges, else DRS_ERR_ARG (drs_crop_dihedral, and drs_crop_resampled below): pointers not NULL (mean3, std3 HOST); n_maps >= 1; C 1..8;
 * ld >= C, a multiple of 4; g 0..7; B, T >= 1, P >= 0, B*(T+2P) <= 65535; drs_crop_resampled: hs, ws >= 1. */
int drs_crop_dihedral(const void* tiles, int tiles_are_f64, const long long* tile_off, const int* tile_h, const int* tile_w, int n_maps,
                      int C, const int* inst, int g, const double* mean3, const double* std3, int B, int T, int P, int ld, float* out,
                      void* stream);
int drs_tile_place_dihedral(float* acc, unsigned int* occur, const float* logits, int h, int w, int K, int T, const int* boxes, int n,
                            int g, void* stream);
/* multi-scale test-time augmentation of overlap-tile inference (opt-in).  For a map X of h x w and a scale s the
 * scaled side is hs = max(1, floor(h s + 0.5)) (ws alike).  D(n -> ns) is bilinear with half-pixel centres (torch interpolate,
 * mode bilinear, align_corners=False, no antialias): per axis, output index d reads
 *     src = max((d + 0.5) (n / ns) - 0.5, 0),  i0 = floor(src),  i1 = min(i0 + 1, n - 1),  l = src - i0
 * and the value is (1-ly)((1-lx) v00 + lx v01) + ly((1-lx) v10 + lx v11).  At ns == n the weights are exactly (1, 0).
 *
 * drs_crop_resampled: conv1's input slab out [B][T+2P][T+2P][ld] of the T x T tiles inst [B][3] = (map, row, col) (device data) of
 * Xs = D(X) -- row / col on the hs x ws grid, every map resampled to hs x ws -- each transformed by the dihedral code g as
 * drs_crop_dihedral transforms it; D in fp64 on every channel, then normalised as drs_crop_normalize normalises (bands 0..2, one
 * rounding to fp32; mean3 / std3 are HOST pointers).  One fused gather: no resized image is made.  Halo and channels C..ld-1 are
 * zero; a tile outside [0, hs-T] x [0, ws-T], or a map index outside [0, n_maps), leaves a zero slab.  At hs == h and ws == w it
 * is drs_crop_dihedral bit for bit (values other than -0.0).
 * drs_resample_accumulate: acc[h][w][K] += U(hs x ws -> h x w) of the class-probability map of src [hs][ws][K]: the vector of a
 * source pixel q is src[q] / occur[q] when src_is_prob (a sum of probabilities), else the max-subtracted fp32 softmax of
 * src[q] / occur[q] as drs_tile_place_dihedral forms it (logits); occur 0 counts as 1.  Coordinates and weights in fp64, the four
 * vectors mixed in fp32 in the order of D above.  K <= 8, h <= 65535.  At hs == h and ws == w it is acc += vector, bit for bit.
 * Ranges, else DRS_ERR_ARG (drs_resample_accumulate): pointers not NULL; K 1..8; hs, ws, h, w >= 1; h <= 65535 (grid.y). */
int drs_crop_resampled(const void* tiles, int tiles_are_f64, const long long* tile_off, const int* tile_h, const int* tile_w, int n_maps,
                       int C, const int* inst, int hs, int ws, int g, const double* mean3, const double* std3, int B, int T, int P, int ld,
                       float* out, void* stream);
int drs_resample_accumulate(const float* src, const unsigned int* occur, int hs, int ws, int K, int src_is_prob, int h, int w, float* acc,
                            void* stream);
/* per-pixel score maps beside the labels (opt-in): drs_stitch_finalize in one pass with up to three uint8 maps.
 * Per pixel i: oc = occur[i] ? occur[i] : 1, v_k = sums[i][k] / oc.
 *   labels[i]      what drs_stitch_finalize writes: the first maximum of the fp64 quotients (bit for bit)
 *   p              sums_are_prob == 0 (sums of logits): the max-subtracted fp32 softmax of v, as drs_resample_accumulate forms it;
 *                  sums_are_prob != 0 (sums of probabilities): p_k = v_k, not renormalised
 *   confidence[i]  p[label]
 *   margin[i]      p[label] - max over k != label of p_k              (K == 1: p[label])
 *   entropy[i]     -sum_k p_k ln p_k / ln K, 0 ln 0 = 0; for logits formed as (ln se - sum_k p_k (v_k - max)) / ln K with se the sum of
 *                  the exponentials, so that no logarithm of an underflowed p_k is taken   (K == 1: 0)
 * Each score s is clamped to [0, 1] and stored as (unsigned char)(int)(255 s + 0.5f).  An uncovered pixel (occur[i] == 0) gets its
 * label as before and confidence 0, margin 0, entropy 255.  Any of the four outputs may be NULL (it is then neither computed for nor
 * written); all four NULL is DRS_ERR_ARG.  K <= 8.
 * Ranges, else DRS_ERR_ARG (and drs_stitch_finalize_scores_t): sums, occur not NULL; one output at least; K 1..8; h, w >= 1. */
int drs_stitch_finalize_scores(const float* sums, const unsigned int* occur, int h, int w, int K, int sums_are_prob,
                               unsigned char* labels, unsigned char* confidence, unsigned char* margin, unsigned char* entropy,
                               void* stream);
/* drs_stitch_finalize_scores at an inverse temperature beta (drs_temperature_stats above: finite, 1/64 <= beta <= 64, else
 * DRS_ERR_ARG).  The labels are drs_stitch_finalize's for every beta: a temperature never moves an arg-max.
 *   beta == 1.0f   runs drs_stitch_finalize_scores: every output is bit for bit that function's; with sums_are_prob that means p is
 *                  NOT renormalised
 *   otherwise      in fp32, with ocf = (float)oc: v_k = s_k / ocf (sums_are_prob == 0) or logf(fmaxf(s_k / ocf, FLT_MIN)) (!= 0);
 *                  t_k = beta v_k, rounded to fp32 BEFORE the maximum is subtracted; p = the max-subtracted softmax of t, the classes
 *                  summed in order, renormalised in BOTH modes; confidence and margin of p as above;
 *                  entropy = (ln se - sum_k p_k (t_k - max t)) / ln K with se the sum of the exponentials, in both modes
 * Uncovered pixels, NULL outputs, the clamp and the byte are drs_stitch_finalize_scores'. */
int drs_stitch_finalize_scores_t(const float* sums, const unsigned int* occur, int h, int w, int K, int sums_are_prob, float beta,
                                 unsigned char* labels, unsigned char* confidence, unsigned char* margin, unsigned char* entropy,
                                 void* stream);
/* local dense-CRF refinement of a whole-map posterior (opt-in; csrc/refine.hip): mean-field iterations of a Potts model
 * with a bilateral and a smoothness kernel (Kraehenbuehl & Koltun, Efficient inference in fully connected CRFs, 2011) over a window of
 * (2R+1)^2 - 1 neighbours dilated by `step` (Teichmann & Cipolla, Convolutional CRFs, 2018).  NORMATIVE: this text and the fp64 numpy
 * statement tests/crf_ref.py.  Inputs are the accumulators handed to drs_stitch_finalize* and the map's image [h][w][C] as the tile
 * pool stores it (fp64 or fp32, each value read as fp32).
 * drs_crf_unary: per pixel i, oc = occur[i] ? occur[i] : 1, in fp32: u_k = sums[i][k] / (float)oc (sums_are_prob == 0) or
 *     logf(fmaxf(sums[i][k] / (float)oc, FLT_MIN)) (!= 0); t_k = beta u_k, rounded before the maximum is subtracted (beta finite,
 *     1/64 <= beta <= 64, else DRS_ERR_ARG);  logp[i][k] = t_k - max t - ln sum_l exp(t_l - max t);  q0[i][k] = softmax_k(t);
 *     live[i] = occur[i] != 0.  A pixel that is not live is dead: it is never a neighbour and no iteration moves its Q.
 * drs_crf_step: one iteration for the image rows [row0, row0 + rows), reading the whole q_in [h*w][K] and writing those rows of q_out
 *     (q_out != q_in).  For a live pixel p the neighbours are q = p + (i, j) step, |i|, |j| <= R, (i, j) != (0, 0), inside the map and live;
 *         kappa(p, q) = w_app exp(-|d|^2 / (2 theta_xy^2) - |f_p - f_q|^2 / (2 theta_rgb^2)) + w_smooth exp(-|d|^2 / (2 theta_s^2)),
 *     d = q - p in pixels, f the C image values;  m_p[k] = sum_q kappa(p, q) q_in[q][k], summed i ascending, then j ascending;
 *         q_out[p] = softmax_k(logp[p][k] + m_p[k]), max-subtracted
 *     (the Potts compatibility; no kernel normalisation).  A dead pixel's q_out is its q_in.  The spatial factors are made once per call
 *     on the host in fp64, the appearance factor is one exp2 per neighbour.  No atomics: a pixel's bits depend neither on the
 *     workgroup tiling nor on how the rows are cut into calls.  Ranges, else DRS_ERR_ARG: K 2..8, C 1..8, R 1..6, step 1..4,
 *     R * step <= 12, w_app, w_smooth finite >= 0, theta_* finite > 0, 0 <= row0, 1 <= rows, row0 + rows <= h.
 * Labels and score maps of the refined posterior: drs_stitch_finalize / drs_stitch_finalize_scores on (Q, live, sums_are_prob = 1).
 * drs_crf_unary ranges, else DRS_ERR_ARG: pointers not NULL; h, w >= 1; K 2..8; beta as above.  drs_crf_step also: pointers not NULL. */
int drs_crf_unary(const float* sums, const unsigned int* occur, int h, int w, int K, int sums_are_prob, float beta, float* logp, float* q0,
                  unsigned int* live, void* stream);
int drs_crf_step(const float* q_in, const float* logp, const unsigned int* live, const void* tile, int tile_is_f64, int C, int h, int w,
                 int K, int row0, int rows, int R, int step, float w_app, float theta_xy, float theta_rgb, float w_smooth, float theta_s,
                 float* q_out, void* stream);
/* multi-scale evaluation (isprs:1347-1474, softmax isprs:38-43): acc[h][w][K] += softmax_k(prob / max(occur, 1));
 * the label map of the summed scales is drs_stitch_finalize(acc, ones, ...). */
int drs_softmax_accumulate(const float* prob, const unsigned int* occur, int h, int w, int K, float* acc, void* stream);
/* boundary-quality counts of a (truth, prediction) pair of label maps (opt-in; csrc/boundary.hip): what trimap
 * accuracy (Kohli et al., Robust higher order potentials, 2009) and Boundary IoU (Cheng et al., CVPR 2021) are sums of.  NORMATIVE:
 * this text and the numpy statement tests/boundary_ref.py.
 * Inputs: truth and pred are uint8 [h][w] on the device; K is the class count, 2 <= K <= 8; ignore_label is -1 for none;
 *     d_0 < d_1 < ... < d_(n-1) are integer distances in pixels, 1 <= n <= 8, 1 <= d_i <= 16; the reach is R = d_(n-1).
 * Distance field: for a byte map m and a pixel p = (y, x),
 *         D2_m(p) = min { dy^2 + dx^2 : |dy| <= R, |dx| <= R, q = p + (dy, dx) inside the map, m[q] != m[p] },
 *     infinite if there is no such q.  Integer arithmetic; nothing is rounded anywhere.  THE EDGE OF THE MAP IS NOT A BOUNDARY:
 *     positions outside the map are never "different" (a mosaic tile cuts objects arbitrarily; Cheng et al.'s implementation pads with
 *     background instead).  A byte is just a byte: in truth a pixel carrying ignore_label differs from every class pixel beside it (in
 *     the ISPRS noBoundary ground truth label 6 is the eroded contour zone, so the distance of a class pixel is measured from the edge
 *     of that zone); in pred, bytes >= K are likewise just different bytes.
 * Bins: bin_m(p) = the smallest i with D2_m(p) <= d_i^2, or n if there is none.  Every pixel has a bin.
 * Table: a pixel is counted exactly when drs_confusion counts it (truth != ignore_label, truth < K, pred < K); for every counted pixel
 *         hist[bin_truth(p)][bin_pred(p)][truth[p]][pred[p]] += 1.
 *     hist = [(n+1)][(n+1)][K][K] 64-bit counters on the device, ADDED to (integer atomics: exact and order-independent), so the maps
 *     of a split accumulate over several calls.  The sum of the table over both bins is drs_confusion's matrix.
 * drs_boundary_distance: d2[y][x] = min(D2_map(p), 65535) as uint16 (infinite -> 65535), R 1..16: the same device function as the
 *     table's, so that a wrong distance field and a wrong count can be told apart.
 * drs_boundary_histogram: the table; distances = n HOST ints.
 * DRS_ERR_ARG (nothing is launched): a null pointer, h or w < 1, h w >= 2^40, K outside 2..8, n outside 1..8, distances that are not
 * strictly ascending or lie outside 1..16, R outside 1..16. */
int drs_boundary_distance(const unsigned char* map, int h, int w, int R, unsigned short* d2, void* stream);
int drs_boundary_histogram(const unsigned char* truth, const unsigned char* pred, int h, int w, int K, int ignore_label,
                           const int* distances, int n, unsigned long long* hist, void* stream);

/* ==================================================================================================================
 * Step level: the reference's three `sess.run` call shapes (isprs:1750-1752 train, :1274-1275 infer, :1588 validate) as entry
 * points, for hosts that do not want to sequence the op-level calls above themselves (csrc/engine.hip).  A drs_net_t holds the
 * net table selected by `net_type` (the reference's if-chain isprs:1660-1680, both spellings of Dilated8Pooling), the variable
 * layout under TensorFlow's scope names and the launch order of a forward pass / a training step.  It owns no device memory:
 *
 *   drs_net_create(...)                                      -> handle
 *   for i < drs_net_num_buffers(h): drs_net_buffer_info(h, i, name, cap, &bytes, &dtype); allocate; drs_net_bind(h, name, ptr, bytes)
 *       (zero-fill "momentum"; fill "params" / "bn" through drs_params_set or directly: layout from drs_net_variable_info)
 *   per step:  drs_crop_normalize(... out = buffer "act:x0" with P, ld from drs_net_layout, out_lab = "labels", out_mask = "acc_mask")
 *              drs_train_step(h, B, S, lr0, flags, global_pixels, stream)     or     drs_forward(h, B, S, flags, ignore_label, stream)
 *   results in the bound buffers: "scalars" (double[4]: [0] mean CE over all ranks, [1] 0.5*sum w^2; total loss = [0] + wd*[1]),
 *       "pred" (u8 [B*S*S]), "logits" (f32 [B*S*S][K], with DRS_WANT_LOGITS), "conf" (i32 [K][K])
 *
 * One stream per handle, not re-entrant per handle, one handle per rank.  Status codes as above; nothing throws.
 * Data parallelism: the sums that must run over all ranks (sync-BN statistics forward and backward, the gradient buffer in
 * buckets, the CE sum, the confusion matrix) go through the callback given to drs_net_set_comm -- the driver owns the
 * communicator (RCCL through torch.distributed in the Python mirror).
 *   allreduce(user, dev_ptr, count, dtype (0 f32, 1 f64, 3 i32), async, stream) -> handle >= 0, or < 0 on failure; in-place sum;
 *       async = 1: may return before the sum is done, the library then calls wait(user, handle, stream) before it reads the data;
 *       async = 0: the sum must be ordered before later work on `stream`.
 *   With a callback installed the sums go through it at world = 1 too (identities there): a single-GPU host can drive the whole
 *   collective path.  world = 1 and no callback: the sums are skipped and batch norm uses its fused single-rank finish.
 */
typedef struct drs_net drs_net_t;
typedef int (*drs_allreduce_fn)(void* user, void* dev_ptr, size_t count, int dtype, int async, void* stream);
typedef int (*drs_wait_fn)(void* user, int handle, void* stream);
#define DRS_WANT_LOGITS 1     /* also write the [B*S*S][K] logits */
#define DRS_WITH_LABELS 2     /* drs_forward: add the confusion matrix of (labels, pred) into "conf" */
#define DRS_USE_ACC_MASK 4    /* gate the confusion matrix by "acc_mask" (augmentation validity / void pixels) */
#define DRS_USE_LOSS_MASK 8   /* drs_train_step: only pixels with loss_mask != 0 enter the loss (contest:881-901) */
#define DRS_NO_UPDATE 16      /* drs_train_step: leave the gradients in "grads", do not apply the momentum update */

int drs_net_create(const char* net_type, int channels, int num_classes, float weight_decay, int b_max, int s_max, int bessel_moving_var,
                   float lr_decay_factor, drs_net_t** out);
void drs_net_destroy(drs_net_t* net);
int drs_net_num_buffers(const drs_net_t* net);
int drs_net_buffer_info(const drs_net_t* net, int index, char* name, int name_cap, size_t* bytes, int* dtype);   /* dtype: 0 f32, 1 f64, 2 u8, 3 i32 */
int drs_net_bind(drs_net_t* net, const char* name, void* dev_ptr, size_t bytes);
int drs_net_buffer(drs_net_t* net, const char* name, void** dev_ptr, size_t* bytes);
int drs_net_layout(const drs_net_t* net, size_t* n_params, size_t* n_decay, size_t* n_bn, int* n_layers, int* x0_channels, int* x0_halo);
/* block `index` of the net as the library runs it (the `_conv_layer` calls of the reference's builder, isprs:761-1086, in order):
 * geom8 = (k, rate, cin, cin_k = input channels the kernel multiplies (conv1: the bands padded to 8), cout, pad_before, pad_after,
 * halo of its input slab); the slabs it reads / writes by name ("x0", "x1", ..., "feat", "concat": buffers "act:<name>"), the
 * channel offset of its output slice (dense / squeeze nets write slices of a shared slab, isprs:921-948), and the pooling after
 * its activation: 0 none, 1 max 3x3 / stride 1, 2 + 256 k = k x k average */
int drs_net_layer_info(const drs_net_t* net, int index, char* name, int name_cap, int* geom8, char* src_slab, char* dst_slab, int slab_cap,
                       int* dst_coff, int* pool);
/* the net as a whole: canonical net_type (aliases resolved), alpha of max(alpha x, x) (0 ReLU, 0.1 leaky ReLU: isprs:620-621), the
 * classifier's input width (isprs:1024-1031), the slab it reads, the topology (0 chain, 1 dense concat isprs:921-948, 2 squeeze
 * isprs:726-742) and the number of squeeze-and-excitation blocks (isprs:1036-1061) */
int drs_net_info(const drs_net_t* net, char* net_type, int name_cap, float* alpha, int* c_last, char* feat_slab, int slab_cap, int* topology,
                 int* n_se);
/* receptive field of the whole net: output pixel p depends on input pixels [p - before, p + after] along each axis (conv SAME pads,
 * + 1 a side per 3 x 3 max-pool, + the SAME pads of a k x k average pool; chain and dense concat sum their blocks, a squeeze stage adds
 * its squeeze block and the larger expand block).  DRS_ERR_ARG for nets with squeeze-and-excitation blocks: their global average over
 * the patch has no finite field. */
int drs_net_receptive_field(const drs_net_t* net, int* before, int* after);
/* the same count with every squeeze-and-excitation layer taken as a per-channel constant (1 x 1): the field of the chains between the
 * gates, which overlap-tile inference with whole-image gates relies on (drs_forward_staged).  Equal to drs_net_receptive_field for a
 * net without such layers; dilated_icpr_rate6_SE: (27, 28). */
int drs_net_receptive_field_gated(const drs_net_t* net, int* before, int* after);
/* squeeze-and-excitation block `index`: scope ("se1": variables <scope>_fc1/weights ...), the block whose activation it scales,
 * channels C and the reduced width C / 4 (isprs:682-697) */
int drs_net_se_info(const drs_net_t* net, int index, char* scope, int scope_cap, int* layer, int* channels, int* reduced);
/* the net_type strings drs_net_create accepts -- the if-chains isprs:1660-1680, coffee:1188-1215, contest:995-1012 -- one per index
 * (DRS_ERR_ARG past the end): the tables, then the aliases; *canonical = index of the table the name resolves to */
int drs_net_type_name(int index, char* name, int name_cap, int* canonical);
/* variables under their TensorFlow scope names (`conv1/weights`, `conv1/biases`, `conv1/moving_mean`, `conv1/moving_variance`,
 * `conv_classifier/weights`, ...: what tf.train.Saver stores, isprs:1693-1695): offset / count in floats inside "params" (and
 * "grads", "momentum") or, with *in_bn = 1, inside "bn"; shape4 = HWIO for kernels */
int drs_net_num_variables(const drs_net_t* net);
int drs_net_variable_info(const drs_net_t* net, int index, char* name, int name_cap, size_t* offset, size_t* count, int* shape4, int* in_bn);
/* copy one variable (slot NULL) or its optimizer accumulator (slot "Momentum") to / from HOST memory; waits for the copy */
int drs_params_get(drs_net_t* net, const char* name, const char* slot, float* host_dst, size_t count, void* stream);
int drs_params_set(drs_net_t* net, const char* name, const char* slot, const float* host_src, size_t count, void* stream);
/* the flat fp32 gradient buffer the RCCL all-reduce runs on (= buffer "grads") */
int drs_grad_buffer(drs_net_t* net, float** dev_ptr, size_t* count);
long long drs_net_global_step(drs_net_t* net, long long set_to);      /* set_to < 0: read only (`main_global_step`, isprs:1685) */
float drs_net_learning_rate(const drs_net_t* net, float lr0);         /* exponential_decay(lr0, global_step, 50000, factor, staircase) */
int drs_net_set_comm(drs_net_t* net, int world, int rank, drs_allreduce_fn allreduce, drs_wait_fn wait, void* user);
/* Library-side collectives (SURVEY 8b `drs_allreduce(handle, comm)`): the sums above issued by the step engine itself through
 * RCCL, bound at run time by dlopen (csrc/rccl_comm.hip) -- no host callback in the step.  comm_small / comm_big: ncclComm_t of
 * `world` ranks on this process's GPU, made by drs_rccl_comm_create below or by the host from the same librccl; comm_big may be
 * NULL.  comm_small carries the latency-bound sums (forward sync-BN statistics on the compute stream itself, backward ones on a
 * side stream under the filter gradient of the block above), comm_big the gradient buckets on comm_stream (hipStream_t; NULL: the
 * library creates one).  The communicators remain the caller's (destroy them after the net).  comm_small = NULL removes the
 * library-side collectives (a net on the drs_net_set_comm callback, or without any communicator, is left as it is); conversely
 * drs_net_set_comm replaces library-side collectives by the callback.  One communicator is never driven from two streams that no
 * event orders: with the two-stream backward pass of small steps (fewer than 2^18 pixels per rank) comm_small stays on the compute
 * stream and every asynchronous sum goes to comm_big; with comm_big = NULL that pass is off.
 * Default form: INLINE -- comm_big is ignored and every sum is issued on the compute stream itself in program order (the sync-BN sums
 * where they are needed, the whole gradient buffer as one all-reduce after the last filter gradient, the loss, the confusion matrix):
 * no side stream, no event, one communicator on one stream.  DRS_RCCL_ASYNC=1 in the environment (read by drs_net_set_rccl) selects
 * the asynchronous form described above (side streams, gradient buckets on comm_big as the layers finish); measured at world 1 its
 * cross-stream hand-overs cost more than the overlap can return on 8 GPUs.
 * A host that binds this ABI directly must have HSA_ENABLE_IPC_MODE_LEGACY=0 in its environment BEFORE the HIP runtime starts
 * (the first HIP call of the process): on this driver RCCL's intra-node transport needs dmabuf IPC and ncclCommInitRank otherwise
 * fails with `hipIpcGetMemHandle: invalid argument` (the Python client and bench.py set it at import).
 *   drs_rccl_bind_library : name the NCCL-API shared library to bind INSTEAD of librccl (another build of RCCL; a test double).  An
 *                         explicit call of the host program, accepted only before anything below has bound a library
 *                         (DRS_ERR_ARG afterwards, or when `path` cannot be loaded): no environment variable substitutes it.
 *   drs_rccl_available : 1 if librccl (or the named library) could be bound.
 *   drs_rccl_unique_id : ncclGetUniqueId into id128 (128 bytes, host memory); rank 0 calls it, the host hands the bytes to every rank.
 *   drs_rccl_comm_create / _destroy : ncclCommInitRank / ncclCommDestroy (collective over the ranks; the device must be current).
 *   drs_rccl_all_reduce : one in-place sum over the ranks on `stream` (dtype as in drs_net_buffer_info: 0 f32, 1 f64, 3 i32) -- the
 *                         call the step engine issues; the host uses it to check a new communicator before handing it over. */
#define DRS_RCCL_FORM_INLINE 1    /* one communicator, every sum on the compute stream in program order (default) */
#define DRS_RCCL_FORM_ASYNC 2     /* DRS_RCCL_ASYNC != 0: two communicators, side streams, an event hand-over per asynchronous sum (r03) */
#define DRS_RCCL_FORM_BUCKETS 3   /* DRS_RCCL_BUCKETS >= 2: inline + the gradient buffer as two all-reduces on comm_big's stream, the first under the rest of the backward pass */
int drs_rccl_form(void);          /* the form drs_net_set_rccl will take, from the environment (the one place that parses it); ASYNC and BUCKETS want comm_big */
int drs_rccl_bind_library(const char* path);
int drs_rccl_available(void);
int drs_rccl_unique_id(unsigned char* id128);
int drs_rccl_comm_create(int world, int rank, const unsigned char* id128, void** comm);
int drs_rccl_comm_destroy(void* comm);
int drs_rccl_all_reduce(void* comm, void* dev_ptr, size_t count, int dtype, void* stream);
int drs_net_set_rccl(drs_net_t* net, int world, int rank, void* comm_small, void* comm_big, void* comm_stream);
int drs_train_step(drs_net_t* net, int B, int S, float lr0, int flags, double global_pixels, void* stream);
int drs_forward(drs_net_t* net, int B, int S, int flags, int ignore_label, void* stream);
int drs_apply_update(drs_net_t* net, float lr0, void* stream);        /* the update alone (after DRS_NO_UPDATE) */
/* overlap-tile inference of a net with n_se squeeze-and-excitation blocks, gated by the mean over the whole IMAGE instead of the patch
 * (opt-in): n_se + 1 sweeps over the tile plan.  Buffers "se_sum<j>" (double [C_j]) and "se_gate<j>" (float [C_j]).
 *   sweep j < n_se : zero "se_sum<j>" on the stream; for every batch of B tiles in "act:x0" drs_forward_staged(stage = j, boxes = the
 *                    B tiles' [B][6] device boxes as drs_tile_place reads them, n_boxes = B): the eval-mode pass up to the block SE j
 *                    follows, SE blocks [0, j) scaling by "se_gate<..>", the block's activated output summed per channel over the
 *                    cores into "se_sum<j>" (drs_se_core_sums).  Then, under data parallelism, one fp64 sum all-reduce of
 *                    "se_sum<j>" by the host, and drs_net_se_gate_finish(j, count = h * w) -> "se_gate<j>" (drs_se_gate).
 *   sweep n_se     : drs_forward_staged(stage = n_se; boxes unused): the whole pass with every gate, "pred" / "logits"
 *                    (DRS_WANT_LOGITS) as drs_forward writes them.
 * DRS_ERR_ARG for a net without squeeze-and-excitation blocks.  drs_forward is not affected. */
int drs_forward_staged(drs_net_t* net, int B, int S, int stage, const int* boxes, int n_boxes, int flags, void* stream);
int drs_net_se_gate_finish(drs_net_t* net, int index, double count, void* stream);
/* the backward pass of drs_train_step on two streams (the filter gradients on a stream of the library's beside the batch-norm-backward /
 * input-gradient chain on `stream`): mode -1 = by the library's rule (steps of fewer than 2^18 pixels; the default), 0 = never (a
 * host that must see every launch of the step on ITS stream), 1 = always.  Bitwise the same step in every mode. */
int drs_net_set_two_streams(drs_net_t* net, int mode);
/* class weights of drs_train_step's loss (drs_classifier_loss_weighted; the "scalars"[0] it leaves is then the weighted mean):
 * host_w = HOST pointer to K = the net's class count finite, non-negative floats, copied into the handle; NULL clears them (the
 * default: the unweighted step, bit for bit).  drs_forward and drs_forward_staged have no loss and ignore them.
 * drs_net_get_class_weights: host_w (K_cap >= K floats) <- the weights in use, ones when none are set; *is_set (may be NULL) says which. */
int drs_net_set_class_weights(drs_net_t* net, const float* host_w, int K);
int drs_net_get_class_weights(const drs_net_t* net, float* host_w, int K_cap, int* is_set);
/* focusing parameter of drs_train_step's loss (drs_classifier_loss_focal; the "scalars"[0] it leaves is then the focal loss, with
 * the class weights when set): 0 (the default: the cross-entropy step, bit for bit) or finite in (0, 8], kept in the handle; anything
 * else DRS_ERR_ARG.  drs_forward and drs_forward_staged have no loss and ignore it. */
int drs_net_set_focal_gamma(drs_net_t* net, float gamma);
int drs_net_get_focal_gamma(const drs_net_t* net, float* gamma);
/* boundary weight of drs_train_step's loss (opt-in; the section "Training level" below states the rule): a in [-1, 64], a == 0 (the
 * default) switches it off -- no new launch, the step is the launches it was, bit for bit; sigma finite in (0, 64]; R in 1..16;
 * anything else DRS_ERR_ARG, also with a == 0.  With a != 0 the step launches drs_patch_boundary_weight(labels, acc_mask if and only
 * if DRS_USE_ACC_MASK, B, S, R, a, 1 / (2 sigma^2)) into the bound buffer "pixel_weight" before the classifier, and the classifier
 * as drs_classifier_loss_pixel with that map; the launch is accounted under the timing kind "classifier_loss".  "scalars"[0] is then
 * the boundary-weighted loss.  drs_forward and drs_forward_staged have no loss and ignore it.
 * drs_net_get_boundary_weight: the triple in use (any pointer may be NULL); (0, 4, 12) when never set. */
int drs_net_set_boundary_weight(drs_net_t* net, double a, double sigma, int R);
int drs_net_get_boundary_weight(const drs_net_t* net, double* a, double* sigma, int* R);
/* soft Dice / Tversky term of drs_train_step's loss (opt-in; the section "Training level: soft Dice / Tversky term" below states the
 * rule): lam in [0, 64], lam == 0 (the default) switches it off -- no new launch, the step is the launches it was, bit for bit; alpha,
 * beta in [0, 1]; smooth finite in (0, 2^20]; anything else DRS_ERR_ARG, also with lam == 0.  With lam != 0 the step, before its fused
 * classifier launch, runs the classifier in its inference form into the bound buffer "logits", drs_patch_dice_coeffs(logits, labels,
 * loss_mask if and only if DRS_USE_LOSS_MASK, ...) into the bound buffers "dice_coef" and "dice_loss", and the classifier as
 * drs_classifier_loss_dice; all of it is accounted under the timing kind "classifier_loss".  The sum of "dice_loss" is added into
 * "scalars"[0] before its all-reduce (count 1, as before) and its scaling by 1 / global pixels: "scalars"[0] is then the cross-entropy
 * part (whatever form is active) + L_dice.  No collective, event or stream is added.  drs_forward and drs_forward_staged have no loss
 * and ignore it.  drs_net_get_dice: the quadruple in use (any pointer may be NULL); (0, 0.5, 0.5, 1) when never set. */
int drs_net_set_dice(drs_net_t* net, double lam, double alpha, double beta, double smooth);
int drs_net_get_dice(const drs_net_t* net, double* lam, double* alpha, double* beta, double* smooth);
/* online hard example mining in drs_train_step's loss (opt-in; the section "Training level: hard example mining" below states the
 * rule): keep finite in (0, 1], keep == 1 (the default) switches it off whatever min_keep is -- no new launch, the step is the launches
 * it was, bit for bit, and the bound buffers "hard_ce" and "pixel_weight" are not touched; min_keep in [0, 2^24); anything else
 * DRS_ERR_ARG, and the pair in use stays.  With keep < 1 the step runs, in this order: the boundary-weight launch if that option is on;
 * the classifier in its inference form into the bound buffer "logits" (ONE such launch when the Dice term is on as well: the two
 * pre-passes share it); drs_patch_dice_coeffs if on; drs_patch_hard_weight(logits, "hard_ce", labels, loss_mask if and only if
 * DRS_USE_LOSS_MASK, ..., "pixel_weight" if the boundary weight is on else NULL, "pixel_weight", NULL); and the classifier as
 * drs_classifier_loss_dice with "pixel_weight" as its pixel map.  All of it is accounted under the timing kind "classifier_loss".
 * "scalars"[0] is then the mined loss: inv_n sum_b (n_b / k_b) sum over the kept pixels of patch b of whatever cross-entropy form is
 * active (+ L_dice over ALL in-loss pixels when that term is on: it is not mined).  The normaliser is unchanged; no collective, event
 * or stream is added.  drs_forward and drs_forward_staged have no loss and ignore it.  drs_net_get_hard_mining: the pair in use
 * (either pointer may be NULL); (1, 0) when never set. */
int drs_net_set_hard_mining(drs_net_t* net, double keep, int min_keep);
int drs_net_get_hard_mining(const drs_net_t* net, double* keep, int* min_keep);
/* Lovasz-softmax term of drs_train_step's loss (opt-in; the section "Training level: Lovasz-softmax term" below states the rule): lam
 * finite in [0, 64], lam == 0 (the default) switches it off -- no new launch, the step is the launches it was, bit for bit (the
 * CLS_DICE path included when only the Dice term is on), and the bound buffers "lovasz_err", "region_grad", "lovasz_loss" and
 * "lovasz_scratch" are not touched; anything else DRS_ERR_ARG, and the value in use stays.  With lam > 0 the step runs, in this order:
 * the boundary-weight launch if that option is on; the classifier in its inference form into the bound buffer "logits" (ONE such
 * launch, shared with the Dice and mining pre-passes); drs_patch_dice_coeffs if on; drs_patch_hard_weight if on;
 * drs_patch_lovasz_grad(logits, "lovasz_err", labels, loss_mask if and only if DRS_USE_LOSS_MASK, ..., "dice_coef" if the Dice term
 * is on else NULL, NULL, "region_grad", "lovasz_loss", "lovasz_scratch", ...); and the classifier as drs_classifier_loss_region with
 * the pixel map, if any, and "region_grad".  All of it is accounted under the timing kind "classifier_loss".  The sums of "dice_loss"
 * (if on) and of "lovasz_loss" are added into "scalars"[0] before its all-reduce: it is then the cross-entropy part (whatever form is
 * active, mined or not) + L_dice (if on) + L_lov; the term itself is never mined or weighted.  No collective, event or stream is
 * added.  drs_forward and drs_forward_staged have no loss and ignore it.  drs_net_get_lovasz: the value in use (the pointer may be
 * NULL); 0 when never set. */
int drs_net_set_lovasz(drs_net_t* net, double lam);
int drs_net_get_lovasz(const drs_net_t* net, double* lam);
/* Boundary (surface) loss of drs_train_step's loss (opt-in; the section "Training level: boundary (surface) loss" below states the
 * rule): lam finite in [0, 64], clip 0 (none) or finite in [1, 32768]; lam == 0 (the default) switches it off -- no new launch, the
 * step is the launches it was, bit for bit, the bound buffers "surface_loss" and "surface_scratch" are not touched, and neither is
 * "region_grad" unless the Lovasz term writes it; anything else DRS_ERR_ARG, and the pair in use stays.  With lam > 0 the step runs,
 * in this order: the boundary-weight launch if that option is on; the classifier in its inference form into the bound buffer "logits"
 * (ONE such launch for all pre-passes); drs_patch_dice_coeffs, drs_patch_hard_weight and drs_patch_lovasz_grad, each if on;
 * drs_patch_surface_loss(logits, labels, loss_mask if and only if DRS_USE_LOSS_MASK, acc_mask if and only if DRS_USE_ACC_MASK (where
 * drs_patch_boundary_weight gets it), ..., lam, clip, dice_coef, accumulate, NULL, "region_grad", "surface_loss", "surface_scratch",
 * ...) with accumulate = 1 and no dice_coef when the Lovasz term is on (its map already holds the Dice part), else "dice_coef" when
 * the Dice term is on, else a plain write; and the classifier as drs_classifier_loss_region with the pixel map, if any, and
 * "region_grad".  All of it is accounted under the timing kind "classifier_loss".  The sum of "surface_loss" is added into
 * "scalars"[0] before its all-reduce, after those of "dice_loss" and "lovasz_loss" (each if on): it is then the cross-entropy part +
 * L_dice (if on) + L_lov (if on) + L_surf; the term itself is never mined or weighted.  No collective, event or stream is added.
 * drs_forward and drs_forward_staged have no loss and ignore it.  drs_net_get_surface_loss: the pair in use (either pointer may be
 * NULL); (0, 0) when never set. */
int drs_net_set_surface_loss(drs_net_t* net, double lam, double clip);
int drs_net_get_surface_loss(const drs_net_t* net, double* lam, double* clip);
/* per-kernel-family HIP-event timing of the launches of a step (bench.py's roofline figures); off by default */
int drs_net_timing(drs_net_t* net, int enable);
int drs_net_num_timing_kinds(void);
int drs_net_timing_summary(drs_net_t* net, int kind, char* name, int name_cap, int* launches, double* ms, double* work);

/* ==================================================================================================================
 * Whole-map level: objects of a finished label map (opt-in; csrc/components.hip).  Connected components, the sieve
 * round that enforces a minimum mapping unit, and the object census.  NORMATIVE: this text and the numpy statement tests/sieve_ref.py.
 * Label-only and integer-only: every output is exact and independent of tiling and scheduling.
 * Inputs: a byte map m, uint8 [h][w] on the device (a byte is just a byte, as in drs_boundary_*); a connectivity c in {4, 8}; a class
 *     count K; K HOST ints min_size[k] >= 0.
 * Components: a component is a maximal c-connected set of pixels that carry the same byte.  label[p] = the smallest linear index
 *     y w + x over the pixels of p's component (int32); size[p] = that component's pixel count (uint32), stored at EVERY pixel of
 *     the component.  The edge of the map connects nothing.
 * Small: a component of byte b is small iff b < K and size < min_size[b].  Bytes >= K are never small, never change, never spread.
 * One round (synchronous: everything is decided on the map as it stands at the start of the round): for a small component S take
 *     every pair (p, q), p in S, q one of p's FOUR edge neighbours inside the map (whatever c is), with m[q] != m[p], m[q] < K and q's
 *     component NOT small.  Each pair offers the key (size[q], 255 - m[q]); S takes the byte of the lexicographically largest key:
 *     the largest non-small neighbour region, ties to the lower class byte.  A small component without such a pair stays as it is in
 *     this round.  All relabelling happens after all keys are chosen.
 * The sieve (the host's loop, loops.sieve_labels): components, then a round, repeated until a round merges nothing or 64 rounds
 *     have run.  Only non-small regions attract, so components only coarsen and the loop ends with no small component
 *     left wherever a non-small component of a byte < K exists; a map without one comes back unchanged.
 * Census: for every component whose byte is < K, table[byte][floor(log2(size))] += 1.
 *
 * drs_components: label and size of map at connectivity 4 or 8 (four launches: tiles in LDS, tile borders on the global forest --
 *     label[] is parent[] --, flatten + count, spread).
 * drs_sieve_scratch_bytes: bytes of drs_sieve_round's scratch for an h x w map (8 h w); 0 outside the ranges.
 * drs_sieve_round: one round from map_in to map_out (map_out == map_in, in place, is allowed); label and size are those of
 *     drs_components on map_in at the caller's connectivity.  The round initialises what it reads of its scratch: the result does
 *     not depend on what the scratch held.  counters = device uint32 [2], STORED: [0] the small components at the start of the
 *     round, [1] those of them that merged.  min_size = K HOST ints, copied into the launch.
 * drs_component_census: table = [K][32] 64-bit device counters, ADDED to.
 * No entry point synchronises: the host reads counters between rounds.
 * Ranges, else DRS_ERR_ARG (nothing is launched, no host pointer is read): pointers not NULL; h, w >= 1, h w <= 2^30; connectivity
 * 4 or 8; 1 <= K <= 32; 0 <= min_size[k] <= 2^30. */
int drs_components(const unsigned char* map, int h, int w, int connectivity, int* label, unsigned int* size, void* stream);
size_t drs_sieve_scratch_bytes(int h, int w);
int drs_sieve_round(const unsigned char* map_in, const int* label, const unsigned int* size, int h, int w, int K, const int* min_size,
                    void* scratch, unsigned char* map_out, unsigned int* counters, void* stream);
int drs_component_census(const unsigned char* map, const int* label, const unsigned int* size, int h, int w, int K,
                         unsigned long long* table, void* stream);
/* Object-level scores of a (truth, prediction) pair of label maps (opt-in; csrc/components.hip): per class, how many
 * truth objects were found, how many predicted objects are spurious and how well the found ones are outlined -- recognition quality,
 * segmentation quality and PQ = SQ RQ (Kirillov et al., Panoptic Segmentation, CVPR 2019, with the connected regions of each class
 * as the segments).  NORMATIVE: this text and the numpy statement tests/objects_ref.py.  Integer-only: every output is exact and
 * independent of tiling and scheduling.
 * Inputs: truth and pred, uint8 [h][w] on the device; K in 1..32; ignore_label, -1 for none; a connectivity c in {4, 8}; (tlabel, tsize)
 *     and (plabel, psize): what drs_components gives for truth and for pred at c.
 * Terms: a truth pixel is COUNTED iff truth != ignore_label and truth < K.  A truth object t is a component of truth whose byte is
 *     counted; |t| = tsize.  A predicted object p is a component of pred with byte < K; |p| = psize.  cover(p) = the number of pixels
 *     of p whose truth pixel is counted.  I(t, p) = |t n p|, used only when t and p carry the same byte.
 *     IoU(t, p) = I / (|t| + cover(p) - I): pixels of p over ignored truth count neither for nor against it.
 * Match: t and p of the same class match iff IoU > 1/2, in integers 3 I > |t| + cover(p).  The match is unique in both directions:
 *     from cover(p) >= I the test gives I > |t| / 2, so at most one p can match a given t; from |t| >= I it gives I > cover(p) / 2, and
 *     the intersections of p with different t are disjoint, so at most one t can match a given p.  No assignment problem arises and
 *     nothing depends on order.
 * Unmatched predicted objects: an unmatched p counts as a predicted object iff 2 cover(p) >= |p|; one that lies mostly over ignored
 *     truth is dropped, as Kirillov et al. drop segments that are mostly void.
 * Outputs of the match (int32 / uint32 [h w], every element stored):
 *     match[i]: i a root of a truth object (tlabel[i] == i, counted): the root of the matched p, or -1; every other i: -2.
 *     inter[i]: root of a matched truth object: I; every other i: 0.
 *     cover[i]: i a root of a predicted object: cover(p); every other i: 0.
 * Table: table[K][4][32], 64-bit device counters, ADDED to, so the maps of a split accumulate; bin(n) = floor(log2 n).
 *     row 0: truth objects by bin(|t|).   row 1: predicted objects by bin(|p|): the matched ones plus the unmatched ones with
 *     2 cover >= |p|.   row 2: matched truth objects by bin(|t|).   row 3: the sum over the matched truth objects, by bin(|t|), of
 *     floor(I 2^20 / (|t| + cover(p) - I)), a 64-bit integer division: exact and order-free.
 * Scores (the host's, metrics.object_scores, fp64), per class and over all classes: TP = sum of row 2, FN = sum of row 0 - TP,
 *     FP = sum of row 1 - TP; precision, recall, RQ = F1 = 2 TP / (2 TP + FP + FN); SQ = sum of row 3 / (TP 2^20); PQ = SQ RQ; recall
 *     per size bin row 2 / row 0.  A class with no truth object and no predicted object has no score.
 *
 * drs_object_scratch_bytes: bytes of drs_object_match's scratch for an h x w map (8 h w: one vote word per pixel); 0 outside the ranges.
 * drs_object_match: match, inter and cover of the pair (four launches: init, the weighted majority vote of every truth object for its
 *     partner, the intersection with the elected candidate, the test).  It initialises what it reads of its scratch: the result does
 *     not depend on what the scratch held.
 * drs_object_table: the table from the outputs of drs_object_match on the same arguments (one launch).
 * No entry point synchronises.  Ranges, else DRS_ERR_ARG (nothing is launched, no pointer is read): pointers not NULL; h, w >= 1,
 * h w <= 2^30; 1 <= K <= 32; -1 <= ignore_label <= 255. */
size_t drs_object_scratch_bytes(int h, int w);
int drs_object_match(const unsigned char* truth, const unsigned char* pred, const int* tlabel, const unsigned int* tsize, const int* plabel,
                     const unsigned int* psize, int h, int w, int K, int ignore_label, void* scratch, int* match, unsigned int* inter,
                     unsigned int* cover, void* stream);
int drs_object_table(const unsigned char* truth, const int* tlabel, const unsigned int* tsize, const unsigned char* pred, const int* plabel,
                     const unsigned int* psize, const int* match, const unsigned int* inter, const unsigned int* cover, int h, int w, int K,
                     int ignore_label, unsigned long long* table, void* stream);
/* Exact Euclidean distance transform of a byte map, and the surface-distance table of a (truth, prediction) pair of label maps on top
 * of it (opt-in; csrc/distance.hip): what the Hausdorff distance at the 95th percentile (HD95), the average symmetric
 * surface distance (ASSD) and the normalised surface Dice at a tolerance (NSD; Nikolov et al. 2018) are sums of.  Unlike
 * drs_boundary_*, whose field is searched inside a window of at most 33 x 33, the transform is UNBOUNDED: a contour 170 pixels off
 * scores as 170 pixels off.  NORMATIVE: this text and the numpy statement tests/surface_ref.py.  Everything is integer arithmetic;
 * nothing is rounded except where stated.
 * Byte read through the veil: b[p] = veil_label where veil != NULL and veil[p] == veil_label, else b[p] = map[p]; veil == NULL: no veil.
 * Sites, by mode: DRS_DT_CLASS: b[p] == cls.  DRS_DT_NOT_CLASS: b[p] != cls.  DRS_DT_CONTOUR: b[p] == cls and at least one of p's four
 *     edge neighbours INSIDE THE MAP has b[q] != cls.  The edge of the map is not a boundary and a byte is just a byte, as in
 *     drs_boundary_*.
 * Distance: d2[y][x] = min over the sites q of (y - qy)^2 + (x - qx)^2, uint32 [h][w] on the device; DRS_DT_INF everywhere when there
 *     is no site.  Exact, with no window: h, w <= 32768 keeps d2 < 2^31.
 * Surface table: table = [2][K][DRS_SURFACE_BINS + 2] 64-bit device counters, ADDED to (integer atomics: exact and order-free), so
 *     the maps of a run accumulate.  pred' = pred veiled by truth at ignore_label (no veil when ignore_label == -1).  For every
 *     class c < K, c != ignore_label: S_t(c) = the DRS_DT_CONTOUR set of c in truth, S_p(c) = that of c in pred'.  Direction 0 walks
 *     the pixels of S_t(c) with their squared distance D to S_p(c); direction 1 walks S_p(c) with D to S_t(c).  Per walked pixel:
 *         the counterpart set is empty:  table[dir][c][BINS + 1] += 1                                       (unsited)
 *         otherwise:                     table[dir][c][min(b, BINS - 1)] += 1  and  table[dir][c][BINS] += f
 *     with b = the smallest integer with 16 D <= b^2 (= ceil(4 d): for an integer tolerance tau, d <= tau iff b <= 4 tau, exactly) and
 *     f = floor(sqrt(D 2^20)) (= floor(1024 d); the operand is below 2^51, a double square root and an integer fix-up give it
 *     exactly).  Bytes >= K in either map are just bytes: they draw contours for their neighbours and have no row of their own.
 * Scores (the host's, metrics.surface_scores, fp64): ASSD = (f of both directions) / 1024 / (sited pixels of both); HD95 = the larger
 *     of the two directions' 95th-percentile bins / 4, rounded UP to a quarter pixel, saturating at (BINS - 1) / 4; NSD at tau =
 *     (pixels of both directions with b <= 4 tau) / (all walked pixels, unsited included).
 *
 * drs_distance_scratch_bytes / drs_surface_scratch_bytes: bytes of scratch for an h x w map (about 10 h w and 31 h w); 0 outside the
 *     ranges.  Every byte of scratch and of d2 that a call reads was written by the same call: results do not depend on what they held.
 * drs_distance_transform: three launches (sites and strip ends down the columns; the distance along the column; the lower envelope of
 *     the parabolas along the rows, Meijster et al. 2000, exact integer separators, columns without a site skipped).
 * drs_surface_histogram: the contours of both maps once, then per class the two transforms in shared launches and one gather;
 *     classes with an empty contour set in either map run no transform (the launches leave at once).  No entry point synchronises.
 * Ranges, else DRS_ERR_ARG (nothing is launched): map / truth, pred, d2, table and scratch not NULL; 1 <= h, w <= 32768, h w <= 2^28;
 * mode 0..2; cls 0..255; veil_label 0..255 when veil is given; scratch_bytes >= the matching query; 2 <= K <= 8; -1 <= ignore_label <= 255. */
#define DRS_DT_CLASS 0
#define DRS_DT_NOT_CLASS 1
#define DRS_DT_CONTOUR 2
#define DRS_DT_INF 0x7fffffff
#define DRS_SURFACE_BINS 4096
size_t drs_distance_scratch_bytes(int h, int w);
int drs_distance_transform(const unsigned char* map, const unsigned char* veil, int veil_label, int h, int w, int mode, int cls,
                           unsigned int* d2, void* scratch, size_t scratch_bytes, void* stream);
size_t drs_surface_scratch_bytes(int h, int w);
int drs_surface_histogram(const unsigned char* truth, const unsigned char* pred, int h, int w, int K, int ignore_label,
                          unsigned long long* table, void* scratch, size_t scratch_bytes, void* stream);
/* Superpixels of a map's image and the vote of a label map inside regions (opt-in; csrc/superpixels.hip): object-
 * based post-processing -- the image is cut into small compact colour-homogeneous segments (SLIC, Achanta et al. 2012) and every
 * connected piece of a segment takes the class most of its pixels, or most of their confidence, voted for.  NORMATIVE: this text and
 * the numpy statement tests/superpixel_ref.py.  After the byte features everything is integer arithmetic and every combination across
 * workgroups an integer atomic add: every output is exact and independent of tiling and scheduling.
 * Features: tile = the map's image [h][w][C] on the device, fp32 or fp64 (tile_is_f64 0 / 1); lo and inv = C HOST floats, copied into
 *     the launch.  Per value v, read as fp32: t = (v - lo[c]) * inv[c], two separately rounded fp32 operations (never one fma);
 *     feat = 0 if !(t > 0) (NaN included), 255 if t >= 255, else (int)rintf(t).  feat = uint8 [h][w][C].
 * Grid: S the grid step, gw = max(1, w / S), gh = max(1, h / S) (floor).  The cell of a pixel: ci = min(gw - 1, x gw / w), cj likewise;
 *     the centre of cell (ci, cj) has id = cj gw + ci.
 * Start: cx = (2 ci + 1) w / (2 gw), cy likewise (floor); the centre's features F are the bytes of the pixel (cx, cy).
 * Assign: the candidates of a pixel are the centres of the up to nine cells (ci + di, cj + dj), |di|, |dj| <= 1, inside the grid.  The
 *     key of a candidate is S^2 sum_c (f_c - F_c)^2 + m^2 ((x - cx)^2 + (y - cy)^2), m the compactness; the pixel takes the candidate
 *     with the smallest key, ties to the lower id.  The key is computed in 32 bits unsigned and is below 2^32: the colour part is at
 *     most 8 255^2 32^2 = 532 684 800; a centre never leaves the 3 x 3 cells around its own (below), a cell is narrower than 2 S, so a
 *     pixel is less than 6 S from a candidate per axis and the spatial part is at most 2 (6 32)^2 40^2 = 117 964 800.
 * Update: per centre with n > 0 assigned pixels, cx, cy and every feature become the rounded mean (2 sum + n) / (2 n) (floor); a
 *     centre with n = 0 keeps its values.  A cluster lies within the 3 x 3 cells around its centre's cell, fewer than 36 864 pixels
 *     with x, y < 32 768: every sum is below 2^32 and is kept in 32 bits.
 * Run: iters times {assign; update}.
 * Outputs: assign = int32 [h][w], the ids of the LAST assign.  centres = int32 [gh gw][C + 3]: (cx, cy, f_0..f_{C-1}, n) after the last
 *     update, n the count of the last assign.  colour = uint8 [h][w], (cj mod 4) 4 + (ci mod 4) of the assigned centre.
 * Colour: a pixel's centre is at most one cell from the pixel's own cell, and the cells of two 4-adjacent pixels differ by at most
 *     one: two 4-adjacent pixels with different centres have centres at most 3 cells apart per axis, so their colours differ.  The
 *     4-connected components of colour are therefore exactly the connected pieces of the clusters: drs_components(colour, 4) labels
 *     them.  A REGION is such a piece; stray fragments are regions of their own and nothing merges them (the sieve's job).
 * Vote: label = what drs_components writes (the smallest pixel index of each pixel's region) -- ANY such labelling, not only
 *     superpixels; weight = uint8 [h][w] or NULL for 1 per pixel.  Per region and class k < K: V[k] = the sum of weight over the
 *     region's pixels whose byte is k (64-bit).  The winner is the largest V, ties to the lower class; if the largest V is 0 the region
 *     stays as it is; otherwise every pixel of the region whose byte is < K takes the winner.  Bytes >= K never vote and never change.
 *
 * drs_superpixel_features: one launch.
 * drs_superpixel_scratch_bytes: bytes of drs_superpixels' scratch (4 gh gw (C + 3): the sums per centre); 0 outside the ranges.
 * drs_superpixels: 1 + 2 iters launches (start; per iteration the assignment with the sums, then the means).  The call initialises
 *     its scratch: the result does not depend on what the scratch held.
 * drs_region_vote_scratch_bytes: bytes of drs_region_vote's scratch for an h x w map (16 h w); 0 outside the ranges.
 * drs_region_vote: from map_in to map_out (map_out == map_in, in place, is allowed).  Region sums are keyed by the region's root: K
 *     passes (one per class, ascending) onto one 64-bit counter per root, each followed by a launch that keeps (sum, class) at the
 *     root where it beats the best so far -- two 64-bit words per pixel, 2 K + 2 launches; the sums of a 32 x 32 tile are
 *     aggregated per region in LDS first, one global atomic add per (region, tile).  It initialises what it reads of its scratch.  counters =
 *     device uint32 [2], STORED: [0] the regions, [1] the pixels whose byte changed.
 * No entry point synchronises.  Ranges, else DRS_ERR_ARG (nothing is launched, no host pointer is read): pointers not NULL (weight
 * may be NULL); tile_is_f64 0 or 1; 1 <= C <= 8; 1 <= h, w <= 32768; 4 <= S <= 32; 1 <= m <= 40; 1 <= iters <= 16; 1 <= K <= 32. */
int drs_superpixel_features(const void* tile, int tile_is_f64, int C, int h, int w, const float* lo, const float* inv,
                            unsigned char* feat, void* stream);
size_t drs_superpixel_scratch_bytes(int C, int h, int w, int S);
int drs_superpixels(const unsigned char* feat, int C, int h, int w, int S, int m, int iters, int* assign, unsigned char* colour,
                    int* centres, void* scratch, void* stream);
size_t drs_region_vote_scratch_bytes(int h, int w);
int drs_region_vote(const unsigned char* map_in, const int* label, const unsigned char* weight, int h, int w, int K, void* scratch,
                    unsigned char* map_out, unsigned int* counters, void* stream);
/* Polygon outlines of a label map (opt-in; csrc/polygons.hip): every region's boundary as closed rings on the pixel-
 * corner lattice, exterior and holes told apart, collinear points dropped.  NORMATIVE: this text and the numpy statement
 * tests/polygon_ref.py.  Integer-only: every output is exact and independent of tiling and scheduling.
 * Input: map = uint8 [h][w] on the device (a byte is just a byte, as for drs_components); a connectivity c, 4 or 8; label = int32
 *     [h][w] of drs_components(map, c).
 * Geometry: pixel (y, x) covers [x, x + 1] x [y, y + 1]; corners are lattice points (X, Y), 0 <= X <= w, 0 <= Y <= h, y down.
 * Cracks: pixel p = y w + x has four directed sides d, each with the pixel on the right-hand side of travel on screen:
 *     d = 0 top, east (x, y) -> (x + 1, y);  1 right, south (x + 1, y) -> (x + 1, y + 1);  2 bottom, west (x + 1, y + 1) -> (x, y + 1);
 *     3 left, north (x, y + 1) -> (x, y).  The pixel across side d is (y - 1, x), (y, x + 1), (y + 1, x), (y, x - 1).  Side d of p is a
 *     CRACK iff the pixel across it is outside the map or carries another byte; its id is e = 4 p + d (h w <= 2^28: int32).  The map
 *     edge IS a crack -- every ring closes --, unlike the scoring ops, where the map edge is not a boundary.
 * Successor of crack (p, d): q = the pixel one step ahead of p in direction d; r = the pixel across side d of q (ahead-left, diagonal
 *     to p); same(.) = inside the map and carrying p's byte.  c = 4: if !same(q) the right turn (p, d + 1), else if !same(r) straight
 *     on (q, d), else the left turn (r, d - 1).  c = 8: if same(r) then (r, d - 1), else if same(q) then (q, d), else (p, d + 1).
 *     d +- 1 mod 4.  The rule is a bijection on the cracks, the head of e is the tail of succ(e), and a cycle stays inside one
 *     c-component.
 * Rings: a ring is a cycle of succ; its id is its smallest crack id (4 label for the exterior ring of a component).  Its VERTICES are
 *     the heads of those of its cracks e with d(succ(e)) != d(e) -- the turning points only --, in cycle order from the first such
 *     crack at or after the ring's smallest crack.  A2 = the sum over its cracks of x0 y1 - x1 y0, tail (x0, y0), head (x1, y1), int64:
 *     the doubled signed area; A2 > 0 an exterior ring, A2 < 0 a hole.  A ring may touch itself at a corner (a pinch at c = 8, a hole
 *     between diagonal pixels at c = 4); that is not repaired.
 * Outputs: ring_table = int64 [rings][7], rings by ascending id: (id, label[id >> 2], map[id >> 2], first vertex, vertex count, crack
 *     count, A2).  vertices = int32 [vertices][2] = (X, Y), ring after ring in table order.
 *
 * drs_polygon_count: two launches; STORES counters[0] (device uint64) = the map's crack count.
 * drs_polygon_scratch_bytes: bytes of the scratch for an h x w map and crack_cap cracks (about 5 h w + 74 crack_cap); 0 outside the
 *     ranges.
 * drs_polygon_rings: builds everything in scratch and STORES counters (device uint64 [4]) = (cracks, rings, vertices, status).  The
 *     crack count is taken from device memory (its own scan), grids are sized by crack_cap.  If the count exceeds crack_cap: status 1,
 *     rings = vertices = 0, nothing outside the scratch and counters is written and the scratch holds no result.  The cracks are
 *     compacted in id order by a scan of the per-pixel counts; ring leaders and positions come from pointer doubling, at most
 *     2 ceil(log2(crack_cap)) + 1 rounds, each a launch that reads only what the launch before it wrote, the launches after a round
 *     that changed nothing returning at once; A2 by 64-bit integer atomic adds.  No kernel waits on another workgroup.  The call
 *     initialises what it reads of its scratch: the result does not depend on what the scratch held.  For measurements: the uint64
 *     words 7 and 8 of the finished scratch hold the rounds the two doublings ran.
 * drs_polygon_write: one launch; writes ring_table and vertices from the scratch of a finished drs_polygon_rings with the same h, w,
 *     crack_cap, and STORES status (device uint32) = 0.  If the scratch holds no result (status 1 above, or another h, w, crack_cap),
 *     or its ring count exceeds ring_cap or its vertex count vertex_cap -- the elements the two outputs have room for --: status = 1
 *     and no output element is written.  A wrong or stale capacity is thus a status word and never a write out of bounds.
 * No entry point synchronises.  Ranges, else DRS_ERR_ARG (nothing is launched, no pointer is read): pointers not NULL; h, w >= 1,
 * h w <= 2^28; connectivity 4 or 8; 1 <= crack_cap <= 4 h w; ring_cap, vertex_cap >= 0. */
int drs_polygon_count(const unsigned char* map, int h, int w, unsigned long long* counters, void* stream);
size_t drs_polygon_scratch_bytes(int h, int w, int crack_cap);
int drs_polygon_rings(const unsigned char* map, const int* label, int h, int w, int connectivity, int crack_cap, void* scratch,
                      unsigned long long* counters, void* stream);
int drs_polygon_write(const void* scratch, int h, int w, int crack_cap, int ring_cap, int vertex_cap, long long* ring_table,
                      int* vertices, unsigned int* status, void* stream);

/* ==================================================================================================================
 * Training level: boundary-weighted cross-entropy (opt-in; csrc/boundary.hip, csrc/pointwise.hip).  A per-pixel weight
 * map that rises towards the nearest pixel of another class (Ronneberger et al., U-Net, 2015: w = 1 + w0 exp(-d^2 / 2 sigma^2)), made
 * from the augmented label patches of a step, and the classifier form that reads it.  NORMATIVE: this text and the numpy statement
 * tests/boundary_weight_ref.py.
 * Inputs: lab, uint8 [B][S][S], the labels the crop kernel wrote; valid, uint8 [B][S][S] or NULL for "all valid"; R in 1..16; a, a
 *     double in [-1, 64]; c = 1 / (2 sigma^2), a double made by the host, sigma in (0, 64].
 * Distance, for patch b and pixel p = (y, x): if valid is given and valid[p] == 0, D2(p) is infinite.  Otherwise
 *     D2(p) = min { dy^2 + dx^2 } over the positions q = p + (dy, dx) with |dy| <= R and |dx| <= R; q inside the same patch,
 *     0 <= qy, qx < S; valid NULL or valid[q] != 0; lab[q] != lab[p].  Infinite if there is no such q.  Integer arithmetic, nothing
 *     is rounded.  As in drs_boundary_*, the edge of the patch is not a boundary and a byte is just a byte.  Patches are independent:
 *     no window reads into the next row's wrap-around or into the next patch.  An invalid q never counts as "different": rotated-in
 *     fill (label 0, mask 0) and void pixels draw no contour along the rotation cut.
 * Weight: w(p) = 1.0f where D2 is infinite (so also at an invalid p, whose treatment by the loss does not change); elsewhere
 *     w(p) = (float)(1.0 + a exp(-D2 c)), evaluated in fp64 and rounded once.  w >= 0 because a >= -1; the tail beyond R is cut to
 *     exactly 1.
 * Loss: with pw the weight map, L = inv_n * sum over the pixels in the loss of pw[p] * wc[y] * m * CE, wc and the focal factor m
 *     exactly those of drs_classifier_loss_focal; the logit gradient is scaled by the same factor pw[p].  Logits, arg-max and the
 *     confusion matrix are not weighted.  inv_n stays the normaliser: no pre-pass, no collective, and the scale of the loss rises with
 *     the mean weight.
 *
 * drs_patch_boundary_weight: weight_out = float [B][S][S]; d2_out = uint16 [B][S][S], min(D2, 65535) (infinite -> 65535), may be NULL:
 *     it exists so that a wrong distance and a wrong weight can be told apart.  One launch, no scratch, no synchronisation.
 *     Ranges, else DRS_ERR_ARG (nothing is launched): lab and weight_out not NULL; B, S >= 1, B S S < 2^24; R in 1..16; a finite in
 *     [-1, 64]; c finite and > 0.
 * drs_classifier_loss_pixel: the arguments of drs_classifier_loss_focal plus pixel_weight, DEVICE float [B S S] or NULL.  With NULL,
 *     or with labels == NULL, it IS drs_classifier_loss_focal: the same launches, every output bit for bit.  Otherwise all three kernel
 *     forms multiply pixel_weight[p] into wc[y] (ones when no class weights are set; the focal form with focal_gamma > 0, else the
 *     weighted one).  The order of every sum is that of the form without a map: it does not depend on the weights.  The weights
 *     themselves are device data and are not checked: the caller keeps them finite and non-negative. */
int drs_patch_boundary_weight(const unsigned char* lab, const unsigned char* valid, int B, int S, int R, double a, double c,
                              unsigned short* d2_out, float* weight_out, void* stream);
int drs_classifier_loss_pixel(const float* feat, int B, int S, int P, int ld, int coff, int C, int K, const float* w,
                              const float* bias, const unsigned char* labels, const unsigned char* loss_mask,
                              const unsigned char* acc_mask, float inv_n, const float* class_weights, float focal_gamma,
                              const float* pixel_weight, float* logits, unsigned char* pred, float* gfeat, int ld_g, int coff_g,
                              float* dw_partial, float* db_partial, double* loss_partial, unsigned int* conf, void* stream);

/* ==================================================================================================================
 * Training level: soft Dice / Tversky term (opt-in; csrc/dice.hip, csrc/pointwise.hip).  A region-overlap term beside
 * the pixel-wise cross-entropy (Milletari et al., V-Net, 2016; Salehi et al., Tversky loss, 2017), per PATCH, so that the loss stays a
 * sum over patches: a sharded batch gives the single-rank loss and gradient with no collective.  NORMATIVE: this text and the numpy
 * statement tests/dice_ref.py.
 * Options: lam finite in (0, 64]; alpha, beta in [0, 1] (0.5, 0.5: Dice); smooth = eps finite in (0, 2^20].
 * "In the loss" means what it means for the cross-entropy: loss_mask set where one is given, and label < K.
 * For patch b and class c, every sum over the in-loss pixels of that patch only, p = softmax(logits):
 *     TP = sum p_c [y = c]      SP = sum p_c      N = sum [y = c]      n_b = sum_c N
 *     D  = TP + alpha (SP - TP) + beta (N - TP) + eps          T = (TP + eps) / D
 *     L_dice = inv_n sum_b n_b (lam / K) sum_c (1 - T)          (inv_n: the step's 1 / global pixels in the loss)
 *     With no mask that is lam times the mean over patches and classes of 1 - T; a patch counts by its share of the pixels in the
 *     loss, and a patch with n_b = 0 contributes nothing (T = 1, coefficients 0).
 * Gradient, for an in-loss pixel of patch b with softmax P and label y:
 *     G_in[b][c]  = -(lam n_b / K) (D - (TP + eps)(1 - beta)) / D^2        G_out[b][c] = +(lam n_b / K) alpha (TP + eps) / D^2
 *     g_c = [y = c] ? G_in[b][c] : G_out[b][c]        dL_dice / dlogit_k = inv_n P_k (g_k - sum_c P_c g_c)
 *     It is ADDED to the logit gradient of whatever cross-entropy form is active.  Class weights, the focal factor and the pixel map
 *     do NOT weight the Dice term.  Logits, arg-max and the confusion matrix are untouched.
 *
 * drs_patch_dice_coeffs: logits = float [B S S][K] (what the classifier's inference form writes), labels = uint8 [B S S], loss_mask =
 *     uint8 [B S S] or NULL.  Out: stats_out = double [B][K][3] (TP, SP, N), may be NULL: it exists so that a wrong sum and a wrong
 *     coefficient can be told apart; coef_out = float [B][K][2] (G_in, G_out), evaluated in fp64 and rounded once; patch_loss_out =
 *     double [B], n_b (lam / K) sum_c (1 - T).  The softmax is fp32 in max-subtracted form, every sum fp64 in a fixed order: no
 *     floating-point atomics, the same bits on every run.  One launch, one workgroup per patch, no scratch.
 *     Ranges, else DRS_ERR_ARG (nothing is launched): logits, labels, coef_out, patch_loss_out not NULL; B, S >= 1, B S S < 2^24; K in
 *     1..8; lam finite in (0, 64]; alpha, beta in [0, 1]; smooth finite in (0, 2^20].
 * drs_classifier_loss_dice: the arguments of drs_classifier_loss_pixel plus dice_coef, DEVICE float [B][K][2] (8-byte aligned, else
 *     DRS_ERR_ARG) or NULL.  With NULL, or with labels == NULL, it IS drs_classifier_loss_pixel: the same launches, every output bit
 *     for bit.  Otherwise all three kernel forms add the term above to the pixel's logit gradients before gfeat, dw_partial and
 *     db_partial are formed; loss_partial stays the cross-entropy sum.  The coefficients are device data and are not checked.
 * drs_dice_loss_add: loss_sum[0] += the sum of patch_loss[0 .. B) (fp64, fixed order) -- how the step joins the patches' terms to the
 *     cross-entropy sum.  patch_loss, loss_sum not NULL, B >= 1, else DRS_ERR_ARG. */
int drs_patch_dice_coeffs(const float* logits, const unsigned char* labels, const unsigned char* loss_mask, int B, int S, int K,
                          double lam, double alpha, double beta, double smooth, double* stats_out, float* coef_out,
                          double* patch_loss_out, void* stream);
int drs_classifier_loss_dice(const float* feat, int B, int S, int P, int ld, int coff, int C, int K, const float* w,
                             const float* bias, const unsigned char* labels, const unsigned char* loss_mask,
                             const unsigned char* acc_mask, float inv_n, const float* class_weights, float focal_gamma,
                             const float* pixel_weight, const float* dice_coef, float* logits, unsigned char* pred, float* gfeat,
                             int ld_g, int coff_g, float* dw_partial, float* db_partial, double* loss_partial, unsigned int* conf,
                             void* stream);
int drs_dice_loss_add(const double* patch_loss, int B, double* loss_sum, void* stream);

/* ==================================================================================================================
 * Training level: hard example mining (opt-in; csrc/hard_mining.hip).  Online hard example mining, also called
 * bootstrapped cross-entropy (Wu et al., Bridging category-level and instance-level semantic segmentation, 2016; Shrivastava et al.,
 * 2016): the cross-entropy of a step runs over the hardest share of each PATCH's pixels only, as the net ranks them at that step.  Per
 * patch, so that the loss stays a sum over patches: a sharded batch gives the single-rank loss and gradient with no collective.
 * NORMATIVE: this text and the numpy statement tests/hard_mining_ref.py.
 * Options: keep finite in (0, 1]; min_keep an integer in [0, 2^24).
 * "In the loss" means what it means for the cross-entropy: loss_mask set where one is given, and label < K.
 * For patch b, every quantity over that patch alone:
 *     n_b = the number of in-loss pixels          k_b = min(n_b, max(ceil(keep n_b), min_keep))    (product and ceil in fp64)
 *     key(p) = log(se) + (max - logit_y), fp32 from the fp32 logits, softmax max-subtracted: se >= 1, key >= +0 -- the PLAIN
 *         cross-entropy: class weights, the focal factor and the pixel map do not move the ranking
 *     kept = the k_b in-loss pixels with the largest keys, ties towards the lower pixel index (a total order: the selection is a
 *         pure function of the keys)
 *     weight_out[p] = kept ? (float)((double)n_b / (double)k_b) * w_in[p] : 0.f       w_in = pixel_weight_in, or 1 without one (one
 *         fp32 multiply; with k_b == n_b the scale is exactly 1 and the map leaves as it came).  n_b == 0: all-zero weights, k_b = 0.
 * The fused classifier multiplies weight_out into the pixel's loss term and gradient like any pixel map (drs_classifier_loss_pixel),
 * so the data term becomes inv_n sum_b (n_b / k_b) sum_{kept p} term(p): each patch contributes the mean of its kept terms, counted
 * by its share of in-loss pixels; inv_n stays 1 / global in-loss pixels.  The selection is a constant in the gradient.
 *
 * drs_patch_hard_weight: logits = float [B S S][K] (what the classifier's inference form writes) or NULL; ce = float [B S S]; labels =
 *     uint8 [B S S]; loss_mask = uint8 [B S S] or NULL; pixel_weight_in = float [B S S] or NULL, and may be weight_out itself (each
 *     element is read and written by the same thread); weight_out = float [B S S]; kept_out = int [B] (k_b) or NULL.
 *     With logits, ce is WRITTEN: the key at in-loss pixels, +0 elsewhere.  With logits == NULL, ce is the INPUT: only in-loss entries
 *     are read, and they must be >= +0 and not NaN -- device data, not checked; a violation gives an unspecified selection but no
 *     access outside the buffers.
 *     An exact radix select of the k_b-th largest key over the fp32 bit pattern (four passes of 8 bits, integer LDS atomics), then a
 *     fixed-order prefix count over the ties: no floating-point atomics, the same bits on every run and every rank.  One launch, one
 *     workgroup per patch, which reads and writes its own patch only; no scratch; any S with B S S < 2^24.
 *     Ranges, else DRS_ERR_ARG (nothing is launched): ce, labels, weight_out not NULL; B, S >= 1, B S S < 2^24; K in 1..8; keep finite
 *     in (0, 1] (1 is legal here: everything is kept, at scale 1); min_keep in [0, 2^24). */
int drs_patch_hard_weight(const float* logits, float* ce, const unsigned char* labels, const unsigned char* loss_mask, int B, int S,
                          int K, double keep, int min_keep, const float* pixel_weight_in, float* weight_out, int* kept_out,
                          void* stream);

/* ==================================================================================================================
 * Training level: Lovasz-softmax term (opt-in; csrc/lovasz.hip, csrc/pointwise.hip).  The convex surrogate of the
 * Jaccard loss itself (Berman, Triki, Blaschko, The Lovasz-softmax loss, CVPR 2018; the paper's classes = 'present'), per PATCH, so
 * that the loss stays a sum over patches: a sharded batch gives the single-rank loss and gradient with no collective.  NORMATIVE: this
 * text and the numpy statement tests/lovasz_ref.py.
 * Option: lam finite in (0, 64].
 * "In the loss" means what it means for the cross-entropy: loss_mask set where one is given, and label < K.
 * Every quantity is per patch b, over its n_b in-loss pixels only.
 *     Error key of class c, fp32 from the fp32 logits: mx = the maximum logit, ex_k = expf(lg_k - mx), se = sum of ex_k in ascending k;
 *         at a pixel with y = c: e_c = (sum_{k != c} ex_k, ascending k) / se  (1 - p_c, never formed by subtraction);
 *         at a pixel with y != c: e_c = ex_c / se.  A true division; 0 <= e <= 1, so a key orders as its bit pattern does.
 *     N_c = #{y = c}; class c is PRESENT in the patch when N_c > 0; C_b = the number of present classes.  Absent classes contribute
 *         nothing.
 *     Order, for a present class: the in-loss pixels by e_c descending, ties towards the lower pixel index (a total order, a pure
 *         function of (key, index)).  For the pixel at 0-based position r: F = the foreground (y = c) pixels before it, Bg = the
 *         background ones; U = N_c + Bg, I = N_c - F (integers).
 *     Jaccard increment at that position, in fp64 from the exact integers: dJ = 1 / U at a foreground pixel, I / (U (U + 1)) at a
 *         background one (J_r - J_{r-1} of the paper's Algorithm 1 without the cancellation; dJ >= 0, and a present class's
 *         increments sum to 1).
 *     Loss_bc = sum_r e_(r) dJ_r (fp64, fixed order)        L_lov = inv_n sum_b (lam n_b / C_b) sum_{c present} Loss_bc
 *         (inv_n: the step's 1 / global pixels in the loss, as for the Dice term)
 * Gradient (the order is a constant): g_c(p) = (lam n_b / C_b) (y_p == c ? -dJ : +dJ); 0 for an absent class and at a pixel not in the
 *     loss; dL_lov / dlogit_k = inv_n P_k (g_k - sum_c P_c g_c), ADDED to the logit gradient of whatever cross-entropy form is active.
 *     Class weights, the focal factor, the boundary map and the mining map do NOT weight the term, and it is not mined.  Logits,
 *     arg-max and the confusion matrix are untouched.
 *
 * drs_lovasz_scratch_bytes: the scratch drs_patch_lovasz_grad needs for (B, S, K) (a multiple of 16, monotone in each argument; 0 for
 *     arguments outside the ranges below): B (K + 1) doubles, and 16 bytes per (pixel, class) where a patch has more pixels than a
 *     workgroup's LDS holds (S > 99).
 * drs_patch_lovasz_grad: logits = float [B S S][K] (what the classifier's inference form writes) or NULL; err = float [B S S][K];
 *     labels = uint8 [B S S]; loss_mask = uint8 [B S S] or NULL.
 *     With logits, err is WRITTEN: the key at in-loss pixels for every class < K, +0 elsewhere.  With logits == NULL, err is the INPUT:
 *     only in-loss entries are read, and they must be in [+0, 1] and not NaN -- device data, not checked; a violation gives an
 *     unspecified order but no access outside the buffers.
 *     dice_coef = float [B][K][2] (drs_patch_dice_coeffs' output, 8-byte aligned) or NULL.  Given, the Dice coefficient is folded in
 *     with one fp32 add: grad_out[p][c] = (float)g_c(p) + (y_p == c ? G_in[b][c] : G_out[b][c]) at in-loss pixels, so that the
 *     classifier needs one map form only.
 *     grad_out = float [B S S][K]: g evaluated in fp64 as ((lam n_b) / C_b) dJ and rounded once; exactly +0 at pixels not in the loss;
 *     at absent classes +0 plus the Dice part, if any.  rank_out = uint32 [B S S][K] or NULL: the 0-based position r, 0xFFFFFFFF where
 *     the pixel is not in the loss or the class is absent -- it exists so that a wrong order and a wrong coefficient can be told
 *     apart.  patch_loss_out = double [B]: (lam n_b / C_b) sum_c Loss_bc, the classes in ascending order; 0 for n_b = 0.
 *     One workgroup per (patch, class), which reads and writes its own patch only: an exact, stable least-significant-digit radix sort
 *     over the key's bit pattern (four passes of 8 bits) carrying the pixel index and the foreground bit; histograms by integer LDS
 *     atomics, positions by ballots and prefix scans in element order, F by a prefix count in sorted order; no floating-point atomics,
 *     every fp64 sum in a fixed order: the same bits on every run and every rank.  Keys and payload stay in LDS up to 9856 pixels per
 *     patch (S <= 99) and ping-pong through scratch above that; any S with B S S < 2^24.  A second, tiny launch joins the classes'
 *     sums.  Scratch is never read before it is written.
 *     Ranges, else DRS_ERR_ARG (nothing is launched): err, labels, grad_out, patch_loss_out not NULL; B, S >= 1, B S S < 2^24; K in
 *     1..8; lam finite in (0, 64]; scratch not NULL, 8-byte aligned, scratch_bytes >= drs_lovasz_scratch_bytes(B, S, K); dice_coef
 *     8-byte aligned.
 * drs_classifier_loss_region: the arguments of drs_classifier_loss_pixel plus region_grad, DEVICE float [B S S][K] (4-byte aligned,
 *     else DRS_ERR_ARG) or NULL.  With NULL, or with labels == NULL, it IS drs_classifier_loss_pixel: the same launches, every output
 *     bit for bit.  Otherwise all three kernel forms add inv_n P_k (g_k - sum_c P_c g_c), g_c = region_grad[p][c], to the in-loss
 *     pixels' logit gradients before gfeat, dw_partial and db_partial are formed -- the arithmetic of drs_classifier_loss_dice with
 *     another source of g: a map that is the Dice coefficients expanded per pixel gives that entry point's outputs bit for bit.
 *     loss_partial stays the cross-entropy sum.  The map is device data and is not checked.
 * The step joins the patches' terms to the cross-entropy sum with drs_dice_loss_add. */
size_t drs_lovasz_scratch_bytes(int B, int S, int K);
int drs_patch_lovasz_grad(const float* logits, float* err, const unsigned char* labels, const unsigned char* loss_mask, int B, int S,
                          int K, double lam, const float* dice_coef, unsigned int* rank_out, float* grad_out, double* patch_loss_out,
                          void* scratch, size_t scratch_bytes, void* stream);
int drs_classifier_loss_region(const float* feat, int B, int S, int P, int ld, int coff, int C, int K, const float* w,
                               const float* bias, const unsigned char* labels, const unsigned char* loss_mask,
                               const unsigned char* acc_mask, float inv_n, const float* class_weights, float focal_gamma,
                               const float* pixel_weight, const float* region_grad, float* logits, unsigned char* pred, float* gfeat,
                               int ld_g, int coff_g, float* dw_partial, float* db_partial, double* loss_partial, unsigned int* conf,
                               void* stream);

/* ==================================================================================================================
 * Training level: boundary (surface) loss (opt-in; csrc/surface_loss.hip).  The boundary loss of Kervadec, Bouchtiba,
 * Desrosiers, Granger, Dolz, Ben Ayed (Boundary loss for highly unbalanced segmentation, MIDL 2019; `SurfaceLoss` in their code): the
 * softmax probability of every class integrated against the class's signed Euclidean distance map of the ground truth -- the
 * quantity the surface-distance validation scores measure, as a term of the loss.  Per PATCH, so that the loss stays a sum over
 * patches: a sharded batch gives the single-rank loss and gradient with no collective.  NORMATIVE: this text and the numpy statement
 * tests/surface_loss_ref.py.
 * Option (lam, clip): lam finite in (0, 64]; clip = 0 (none) or finite in [1, 32768] pixels.
 * Every quantity is per patch b and independent of other patches.
 *     A pixel is COUNTED when label < K, loss_mask is set where one is given, and valid is set where one is given.  Pixels that are
 *         not counted (rotated-in fill, void) are never a site and carry no term.
 *     Sites of class c: A_c = the counted pixels with y = c, O_c = the counted pixels with y != c.  If either set is empty, phi_c = 0
 *         in the whole patch (an absent class, and a class without a contour in the patch).
 *     Signed squared distance, exact integers; the patch's edge is no boundary and nothing reads across patches:
 *         at p in O_c: D2 = min_{q in A_c} |p - q|^2, phi_c(p) = +sqrt(D2);
 *         at p in A_c: D2 = min_{q in O_c} |p - q|^2, phi_c(p) = 1 - sqrt(D2)   (the published -(sqrt(D2) - 1); +0 where D2 = 1);
 *         phi = 0 at pixels that are not counted.  On a fully counted patch this is edt(~pos) ~pos - (edt(pos) - 1) pos of the
 *         published code, with scipy's distance_transform_edt.
 *     Map: g_c(p) = (float)(lam clamp(phi_c(p), -clip, +clip)); the square root and the product in fp64, rounded once; exactly +0
 *         where phi is 0.
 *     Loss: L_surf = inv_n sum_b sum_{p counted} sum_c g_c(p) P_c(p); P_c = ex_c / se in fp32 from the fp32 logits (mx = the maximum
 *         logit, ex_k = expf(lg_k - mx), se = sum of ex_k in ascending k, a true division), the products and sums in fp64 in a fixed
 *         order (inv_n: the step's 1 / global pixels in the loss, as for the Dice and Lovasz terms).
 * Gradient: dL_surf / dlogit_k = inv_n P_k (g_k - sum_c P_c g_c), ADDED to the logit gradient of whatever cross-entropy form is
 *     active -- what drs_classifier_loss_region adds for the map g.  Class weights, the focal factor, the boundary map and the mining
 *     map do NOT weight the term, and it is not mined.  Logits, arg-max and the confusion matrix are untouched.
 *
 * drs_surface_loss_scratch_bytes: the scratch drs_patch_surface_loss needs for (B, S, K) (a multiple of 16, monotone in each argument;
 *     0 for arguments outside the ranges below): B K doubles (rounded up to 16 bytes), and above S = 128 the two column-distance
 *     planes, 4 S S bytes (rounded up to 16) per (patch, class).
 * drs_patch_surface_loss: logits = float [B S S][K] (what the classifier's inference form writes) or NULL -- then only the map and
 *     phi2_out are made and patch_loss_out is written as 0; labels = uint8 [B S S]; loss_mask, valid = uint8 [B S S] or NULL.
 *     phi2_out = int32 [B S S][K] or NULL: +D2 outside (p in O_c), -D2 inside (p in A_c), 0 where phi_c = 0 in the patch or the pixel
 *     is not counted -- it exists so that a wrong distance and a wrong coefficient can be told apart.
 *     grad_io = float [B S S][K].  accumulate == 0: WRITTEN, g_c(p) at counted pixels and +0 elsewhere; with dice_coef = float
 *     [B][K][2] (drs_patch_dice_coeffs' output, 8-byte aligned) the Dice coefficient is folded in with one fp32 add at the pixels
 *     that are in the loss (label < K and loss_mask set, whatever valid says), as drs_patch_lovasz_grad does:
 *     grad_io[p][c] = g_c(p) + (y_p == c ? G_in[b][c] : G_out[b][c]), so that the classifier reads one map form only.
 *     accumulate != 0: g_c(p) is ADDED to what grad_io holds with one fp32 add at counted pixels, every other entry is left alone --
 *     how the step stacks the term on drs_patch_lovasz_grad's map.  dice_coef together with accumulate: DRS_ERR_ARG.
 *     patch_loss_out = double [B]: sum_c sum_p g_c(p) P_c(p), the classes in ascending order; 0 for a patch with nothing counted.
 *     One workgroup per (patch, class), which reads and writes its own patch only: the label / counted bytes, then one thread per
 *     column leaves the distance to the nearest site of the column for both site sets (uint16, 0xFFFF: none; a sweep down and one
 *     up), then every thread takes pixels, lanes on consecutive x, and scans its row outward from x for min_i (x - i)^2 + g[y][i]^2,
 *     four offsets to either side per round (their reads in flight together), until a round's first offset squared alone reaches the
 *     best so far.  Exact.  The planes and bytes stay in LDS up to S = 128 (5 S S bytes) and the
 *     planes live in scratch above that; any S with B S S < 2^24.  No floating-point atomics, every fp64 sum in a fixed order: the
 *     same bits on every run and every rank.  A second, tiny launch joins the classes' sums.  Scratch is never read before it is
 *     written.
 *     Ranges, else DRS_ERR_ARG (nothing is launched): labels, grad_io, patch_loss_out not NULL; B, S >= 1, B S S < 2^24; K in 1..8;
 *     lam finite in (0, 64]; clip 0 or finite in [1, 32768]; scratch not NULL, 8-byte aligned, scratch_bytes >=
 *     drs_surface_loss_scratch_bytes(B, S, K); dice_coef and patch_loss_out 8-byte aligned; logits, grad_io, phi2_out 4-byte aligned.
 * The step joins the patches' terms to the cross-entropy sum with drs_dice_loss_add. */
size_t drs_surface_loss_scratch_bytes(int B, int S, int K);
int drs_patch_surface_loss(const float* logits, const unsigned char* labels, const unsigned char* loss_mask,
                           const unsigned char* valid, int B, int S, int K, double lam, double clip, const float* dice_coef,
                           int accumulate, int* phi2_out, float* grad_io, double* patch_loss_out, void* scratch, size_t scratch_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DRS_H_ */
