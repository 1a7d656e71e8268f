// The data-dependent pre-pass of the soft Dice / Tversky term of the training loss (opt-in; include/drs.h, "Training level: soft
// Dice / Tversky term"; tests/dice_ref.py states the rule in numpy).  The gradient of the term at a pixel depends on
// sums over the pixel's whole patch, so the step runs the classifier once in its inference form, this kernel over the logits, and
// then the fused classifier with the per-(patch, class) coefficients this kernel leaves (csrc/pointwise.hip, CLS_DICE).
//   per patch b and class c, over the pixels of the patch that are in the loss (loss_mask set when given, label < K), p = softmax:
//     TP = sum p_c [y = c]    SP = sum p_c    N = sum [y = c]    n_b = sum_c N
//     D = TP + alpha (SP - TP) + beta (N - TP) + eps        T = (TP + eps) / D
//     G_in  = -(lam n_b / K) (D - (TP + eps)(1 - beta)) / D^2      (dL / dp_c at a pixel whose label is c)
//     G_out = +(lam n_b / K) alpha (TP + eps) / D^2                (at a pixel whose label is another class)
//     patch_loss = n_b (lam / K) sum_c (1 - T)
// The softmax is fp32, max-subtracted, from the fp32 logits (expf and a true division: this pass is a few microseconds, nothing here
// is worth a fast intrinsic); every sum is fp64 in a fixed order -- a thread's pixels in ascending order, the 64 lanes of a wave by a
// butterfly, the four waves in wave order -- so a launch gives the same bits every time.  No atomics.
#include "drs_common.hpp"
#include "../../include/drs.h"
#include <cmath>

namespace {

struct DiceArgs {
  const float* logits;               // [B * SS][K]
  const unsigned char* labels;       // [B * SS]
  const unsigned char* loss_mask;    // [B * SS] or null
  int SS;
  double lam, alpha, beta, smooth;
  double* stats;                     // [B][K][3] or null
  float* coef;                       // [B][K][2]
  double* patch_loss;                // [B]
};

// One workgroup per patch (B = 128 patches of 4096 pixels: half the CUs for a few microseconds).  KM = the class count, known at
// compile time so that a thread's 2 K running sums stay in registers.
template <int KM>
__global__ void __launch_bounds__(256) patch_dice_coeffs_kernel(const DiceArgs a) {
  __shared__ double red[4][KM][2];
  __shared__ int redn[4][KM];
  __shared__ double one_minus_t[KM];
  __shared__ double n_patch;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x;
  const int base = b * a.SS;              // (B SS < 2^24: every index fits an int)
  double tp[KM], sp[KM];
  int cnt[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) { tp[k] = 0.0; sp[k] = 0.0; cnt[k] = 0; }
  for (int i = t; i < a.SS; i += 256) {
    const int p = base + i;
    const int y = a.labels[p];
    if ((a.loss_mask && !a.loss_mask[p]) || y >= KM) continue;
    float lg[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) lg[k] = a.logits[(size_t)p * KM + k];
    float mx = lg[0];
#pragma unroll
    for (int k = 1; k < KM; ++k) mx = lg[k] > mx ? lg[k] : mx;
    float ex[KM], se = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) { ex[k] = expf(lg[k] - mx); se += ex[k]; }
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const double pk = (double)(ex[k] / se);
      sp[k] += pk;
      if (k == y) { tp[k] += pk; cnt[k] += 1; }
    }
  }
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    double v0 = tp[k], v1 = sp[k];
    int c = cnt[k];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      v0 += __shfl_xor(v0, d);
      v1 += __shfl_xor(v1, d);
      c += __shfl_xor(c, d);
    }
    if (lane == 0) { red[wave][k][0] = v0; red[wave][k][1] = v1; redn[wave][k] = c; }
  }
  __syncthreads();
  if (t < KM) {
    const double TP = ((red[0][t][0] + red[1][t][0]) + red[2][t][0]) + red[3][t][0];
    const double SP = ((red[0][t][1] + red[1][t][1]) + red[2][t][1]) + red[3][t][1];
    int nb = 0, nk = 0;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      const int c = ((redn[0][k] + redn[1][k]) + redn[2][k]) + redn[3][k];
      nb += c;
      nk = k == t ? c : nk;
    }
    const double N = (double)nk;
    const double D = TP + a.alpha * (SP - TP) + a.beta * (N - TP) + a.smooth;
    const double T = (TP + a.smooth) / D;
    const double f = a.lam * (double)nb / (double)KM;
    const size_t o = (size_t)b * KM + t;
    // (a patch with no pixel in the loss: T = eps / eps = 1 and both coefficients exactly +0)
    a.coef[2 * o] = nb ? (float)(-f * (D - (TP + a.smooth) * (1.0 - a.beta)) / (D * D)) : 0.f;
    a.coef[2 * o + 1] = nb ? (float)(f * a.alpha * (TP + a.smooth) / (D * D)) : 0.f;
    if (a.stats) { a.stats[3 * o] = TP; a.stats[3 * o + 1] = SP; a.stats[3 * o + 2] = N; }
    one_minus_t[t] = 1.0 - T;
    if (t == 0) n_patch = (double)nb;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < KM; ++k) s += one_minus_t[k];
    a.patch_loss[b] = n_patch * (a.lam / (double)KM) * s;
  }
}

// out[0] += the sum of in[0 .. n): a thread's elements in ascending order, then a tree over the 256 threads
__global__ void __launch_bounds__(256) add_sum_f64_kernel(const double* __restrict__ in, int n, double* __restrict__ out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += in[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] += sh[0];
}

template <int KM>
void dice_launch(int K, int B, hipStream_t st, const DiceArgs& a) {
  if constexpr (KM < 8)
    if (K != KM) return dice_launch<KM + 1>(K, B, st, a);
  DRS_LAUNCH(patch_dice_coeffs_kernel<KM>, dim3(B), dim3(256), 0, st, a);
}

}  // namespace

extern "C" {

int drs_patch_dice_coeffs(const float* logits, const unsigned char* labels, const unsigned char* loss_mask, int B, int S, int K,
                          double lam, double alpha, double beta, double smooth, double* stats_out, float* coef_out,
                          double* patch_loss_out, void* stream) {
  if (!logits || !labels || !coef_out || !patch_loss_out) return DRS_ERR_ARG;
  if (B < 1 || S < 1 || (long long)B * S * S >= (1LL << 24) || K < 1 || K > 8) return DRS_ERR_ARG;
  if (!std::isfinite(lam) || !(lam > 0.0) || lam > 64.0 || !(alpha >= 0.0 && alpha <= 1.0) || !(beta >= 0.0 && beta <= 1.0)) return DRS_ERR_ARG;
  if (!std::isfinite(smooth) || !(smooth > 0.0) || smooth > 1048576.0) return DRS_ERR_ARG;
  DiceArgs a;
  a.logits = logits; a.labels = labels; a.loss_mask = loss_mask; a.SS = S * S;
  a.lam = lam; a.alpha = alpha; a.beta = beta; a.smooth = smooth;
  a.stats = stats_out; a.coef = coef_out; a.patch_loss = patch_loss_out;
  dice_launch<1>(K, B, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

int drs_dice_loss_add(const double* patch_loss, int B, double* loss_sum, void* stream) {
  if (!patch_loss || !loss_sum || B < 1) return DRS_ERR_ARG;
  DRS_LAUNCH(add_sum_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, patch_loss, B, loss_sum);
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
