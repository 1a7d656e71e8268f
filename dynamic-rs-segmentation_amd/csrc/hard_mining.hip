// The data-dependent pre-pass of online hard example mining (bootstrapped cross-entropy) in the training loss (opt-in; include/drs.h,
// "Training level: hard example mining"; tests/hard_mining_ref.py states the rule in numpy).  The cross-entropy of a
// mined step runs over the hardest share of each patch's pixels only, so the step runs the classifier once in its inference form,
// this kernel over the logits, and then the fused classifier with the per-pixel weight map this kernel leaves: 0 at a pixel that is
// left out, n_b / k_b at one that is kept (times the incoming map, when there is one).  The classifier kernels do not change.
//   per patch b, over the pixels of the patch that are in the loss (loss_mask set when given, label < K):
//     n_b = their number          k_b = min(n_b, max(ceil(keep n_b), min_keep))         (fp64 product and ceil)
//     key = log(se) + (max - logit_y)     fp32, softmax max-subtracted: se >= 1 and key >= +0
//     kept = the k_b largest keys, ties towards the lower pixel index
// A non-negative float orders as its bit pattern does as an unsigned integer, so the k_b-th largest key is found EXACTLY by a radix
// select over the bits: four passes of 8 bits from the top, each a 256-bin histogram in LDS (integer atomics: the counts do not
// depend on their order) of the keys that agree with the digits chosen so far, and a suffix count over the bins in a fixed order.
// Every key above the threshold T is kept; of the keys equal to T the first k_b - #{key > T} in pixel order are, by a prefix count
// over the workgroup in pixel order (ballot and popcount inside a wave, the four waves in wave order).  No floating-point atomics, no
// floating-point sums: a launch gives the same bits every time.  Keys are re-read from `ce` in every pass (a thread reads what it
// wrote itself), so the patch side is not bounded by registers or LDS.
#include "drs_common.hpp"
#include "../../include/drs.h"
#include <cmath>

namespace {

struct HardArgs {
  const float* logits;               // [B * SS][K] or null: `ce` is then the input
  float* ce;                         // [B * SS]
  const unsigned char* labels;       // [B * SS]
  const unsigned char* loss_mask;    // [B * SS] or null
  int SS;
  double keep;
  int min_keep;
  const float* w_in;                 // [B * SS] or null; may be weight_out (each element is read and written by the same thread)
  float* w_out;                      // [B * SS]
  int* kept;                         // [B] or null
};

// exclusive prefix of v over the 256 threads in thread order, and the total: lane scan by shuffles, then the four waves in wave order.
// wsum: 4 ints of LDS that nobody else touches until the caller's next barrier
__device__ __forceinline__ int block_prefix(int v, int lane, int wave, int* wsum, int& total) {
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d);
    if (lane >= d) inc += u;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  const int w0 = wsum[0], w1 = wsum[1], w2 = wsum[2], w3 = wsum[3];
  total = ((w0 + w1) + w2) + w3;
  const int before = wave == 0 ? 0 : wave == 1 ? w0 : wave == 2 ? w0 + w1 : (w0 + w1) + w2;
  return before + inc - v;
}

// One workgroup per patch (B = 128 patches of 4096 pixels: half the CUs for a few microseconds).  KM = the class count, known at
// compile time so that a pixel's logits stay in registers.
template <int KM>
__global__ void __launch_bounds__(256) patch_hard_weight_kernel(const HardArgs a) {
  __shared__ int hist[256];
  __shared__ int wsum[2][4];
  __shared__ int sel[2];             // the digit chosen in a pass, and how many keys are still wanted inside its bin
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x;
  const int base = b * a.SS;              // (B SS < 2^24: every index fits an int)
  const int rounds = (a.SS + 255) >> 8;   // pixel i of the patch belongs to thread i % 256, in round i / 256
  auto in_loss = [&](int p) { return !(a.loss_mask && !a.loss_mask[p]) && a.labels[p] < KM; };

  // (A) the keys and n_b
  int cnt = 0;
  for (int i = t; i < a.SS; i += 256) {
    const int p = base + i;
    const bool in = in_loss(p);
    cnt += in ? 1 : 0;
    if (a.logits) {
      float key = 0.f;
      if (in) {
        const int y = a.labels[p];
        float lg[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) lg[k] = a.logits[(size_t)p * KM + k];
        float mx = lg[0], ly = lg[0];
#pragma unroll
        for (int k = 1; k < KM; ++k) { mx = lg[k] > mx ? lg[k] : mx; ly = k == y ? lg[k] : ly; }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < KM; ++k) se += expf(lg[k] - mx);
        key = logf(se) + (mx - ly);
      }
      a.ce[p] = key;
    }
  }
  int nb;
  block_prefix(cnt, lane, wave, wsum[0], nb);
  if (nb == 0) {                          // (the same for every thread) nothing is in the loss: all-zero weights, nothing is divided
    for (int i = t; i < a.SS; i += 256) a.w_out[base + i] = 0.f;
    if (t == 0 && a.kept) a.kept[b] = 0;
    return;
  }
  int kb = (int)ceil(a.keep * (double)nb);
  kb = kb > a.min_keep ? kb : a.min_keep;
  kb = kb < nb ? kb : nb;                 // 1 <= kb <= nb: keep > 0 and nb >= 1

  // (B) the kb-th largest key: T = prefix after four digits; `want` ends as the number of keys equal to T that are kept (>= 1)
  unsigned prefix = 0u, mask = 0u;
  int want = kb;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < a.SS; i += 256) {
      const int p = base + i;
      if (!in_loss(p)) continue;
      const unsigned u = __float_as_uint(a.ce[p]);
      if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);
    }
    __syncthreads();
    // thread t looks at digit 255 - t: `above` = the candidates with a larger digit.  At least `want` candidates exist, so exactly
    // one digit has above < want <= above + c
    const int c = hist[255 - t];
    int total;
    const int above = block_prefix(c, lane, wave, wsum[(shift >> 3) & 1], total);
    if (above < want && want <= above + c) { sel[0] = 255 - t; sel[1] = want - above; }
    __syncthreads();
    prefix |= (unsigned)sel[0] << shift;
    mask |= 255u << shift;
    want = sel[1];
    // (the next pass writes hist and sel only behind its own first barrier, which every thread reaches after these reads)
  }

  // (C) + (D) in pixel order: every key above T, and the first `want` keys equal to T
  const float scale = (float)((double)nb / (double)kb);
  int seen = 0;                           // keys equal to T in the rounds before this one
  for (int r = 0; r < rounds; ++r) {
    const int i = (r << 8) + t;
    const int p = base + i;
    bool in = false, tie = false, kept = false;
    if (i < a.SS && in_loss(p)) {
      const unsigned u = __float_as_uint(a.ce[p]);
      in = true; tie = u == prefix; kept = u > prefix;
    }
    int total = 0, rank = 0;
    if (seen < want) {                    // (the same for every thread) later ties are all left out
      rank = seen + block_prefix(tie ? 1 : 0, lane, wave, wsum[r & 1], total);
      kept = kept || (tie && rank < want);
      seen += total;
    }
    if (i < a.SS) {
      float w = 0.f;
      if (in && kept) w = a.w_in ? scale * a.w_in[p] : scale;
      a.w_out[p] = w;
    }
  }
  if (t == 0 && a.kept) a.kept[b] = kb;
}

template <int KM>
void hard_launch(int K, int B, hipStream_t st, const HardArgs& a) {
  if constexpr (KM < 8)
    if (K != KM) return hard_launch<KM + 1>(K, B, st, a);
  DRS_LAUNCH(patch_hard_weight_kernel<KM>, dim3(B), dim3(256), 0, st, a);
}

}  // namespace

extern "C" {

int drs_patch_hard_weight(const float* logits, float* ce, const unsigned char* labels, const unsigned char* loss_mask, int B, int S,
                          int K, double keep, int min_keep, const float* pixel_weight_in, float* weight_out, int* kept_out,
                          void* stream) {
  if (!ce || !labels || !weight_out) return DRS_ERR_ARG;
  if (B < 1 || S < 1 || (long long)B * S * S >= (1LL << 24) || K < 1 || K > 8) return DRS_ERR_ARG;
  if (!std::isfinite(keep) || !(keep > 0.0) || keep > 1.0 || min_keep < 0 || min_keep >= (1 << 24)) return DRS_ERR_ARG;
  HardArgs a;
  a.logits = logits; a.ce = ce; a.labels = labels; a.loss_mask = loss_mask; a.SS = S * S;
  a.keep = keep; a.min_keep = min_keep; a.w_in = pixel_weight_in; a.w_out = weight_out; a.kept = kept_out;
  hard_launch<1>(K, B, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
