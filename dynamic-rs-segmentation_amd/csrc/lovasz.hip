// The data-dependent pre-pass of the Lovasz-softmax term of the training loss (opt-in; include/drs.h, "Training level: Lovasz-softmax
// term"; tests/lovasz_ref.py states the rule in numpy).  The gradient of the term at a pixel depends on where the pixel
// ranks among its patch's errors for each class, so the step runs the classifier once in its inference form, this pre-pass over the
// logits, and then the fused classifier with the per-(pixel, class) map this pre-pass leaves (csrc/pointwise.hip, CLS_REGION).
//   per patch b and class c, over the n_b pixels of the patch that are in the loss (loss_mask set when given, label < K):
//     e_c   = (sum_{k != c} ex_k) / se  at a pixel with y = c,  ex_c / se  elsewhere      (fp32, max-subtracted, ascending k)
//     order = e_c descending, ties towards the lower pixel index; r the 0-based position, F / Bg the foreground (y = c) / background
//             pixels before it, N_c the foreground pixels of the patch, U = N_c + Bg, I = N_c - F
//     dJ    = 1 / U at a foreground pixel,  I / (U (U + 1)) at a background one          (fp64 from exact integers)
//     g_c(p) = (lam n_b / C_b) (y_p == c ? -dJ : +dJ)      Loss_bc = sum_r e_(r) dJ_r      C_b = the classes with N_c > 0
// One workgroup per (patch, class).  0 <= e <= 1, so a key orders as its bit pattern does: the workgroup sorts the pixels of its patch
// by 0x3F800000 - bits(e) ascending (a pixel that is not in the loss carries 0xFFFFFFFF and sorts behind all of them) with a STABLE
// least-significant-digit radix sort, four passes of 8 bits, carrying the pixel index, the foreground bit and the in-loss bit; the
// input order is the pixel order, so ties end up towards the lower index.  In a pass every wave owns a contiguous quarter of the
// elements: a 256-bin histogram per wave (integer LDS atomics: counts do not depend on their order), an exclusive scan over
// (digit, wave) in that order, and then the wave walks its quarter in element order, 64 at a time -- the position of an element is its
// wave's running offset for the digit plus the number of lower lanes with the same digit (eight ballots).  No position comes from an
// atomic.  F is a prefix count over the workgroup in sorted order; every fp64 sum is in a fixed order; no floating-point atomics: a
// launch gives the same bits every time.  Keys and payload sit in LDS while the patch has at most LOV_LDS_ELEMS pixels (16 bytes per
// pixel: two ping-pong pairs), in the caller's scratch above that.  The classes' sums meet in a second, tiny launch.
#include "drs_common.hpp"
#include "../../include/drs.h"
#include <cmath>
#include <cstdint>

namespace {

constexpr int LOV_LDS_ELEMS = 9856;                   // 154 KiB of the 160 KiB a workgroup may take; the rest: histograms and sums
constexpr size_t LOV_LDS_BYTES = (size_t)LOV_LDS_ELEMS * 16;
constexpr unsigned LOV_FG = 0x80000000u, LOV_IN = 0x40000000u, LOV_IDX = 0x00FFFFFFu, LOV_ONE = 0x3F800000u;

struct LovArgs {
  const float* logits;               // [B * SS][K] or null: `err` is then the input
  float* err;                        // [B * SS][K]
  const unsigned char* labels;       // [B * SS]
  const unsigned char* loss_mask;    // [B * SS] or null
  int SS;
  double lam;
  const float* dice;                 // [B][K][2] or null
  unsigned* rank;                    // [B * SS][K] or null
  float* grad;                       // [B * SS][K]
  double* cls_loss;                  // scratch [B][K]: Loss_bc (0 for an absent class)
  double* factor;                    // scratch [B]: lam n_b / C_b (0 for an empty patch)
  double* patch_loss;                // [B]
  unsigned* pp;                      // scratch [B K][4][SS]: the ping-pong pairs of the form without LDS storage
};

// exclusive prefix of v over the 256 threads in thread order, and the total: lane scan by shuffles, then the four waves in wave order.
// wsum: 4 ints of LDS that nobody else touches until the caller's next barrier
__device__ __forceinline__ int lov_block_prefix(int v, int lane, int wave, int* wsum, int& total) {
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

template <int KM, bool INLDS>
__global__ void __launch_bounds__(256) patch_lovasz_kernel(const LovArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned lov_lds[];      // [4][SS] when INLDS
  __shared__ int hist[4][256];
  __shared__ int wsum[2][4];
  __shared__ int ncls[8];
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x / KM, c = blockIdx.x - b * KM;
  const int n = a.SS;
  const int base = b * n;                 // (B SS < 2^24: every pixel index fits an int)
  unsigned* q;
  if constexpr (INLDS) q = lov_lds;
  else q = a.pp + (size_t)blockIdx.x * 4 * (size_t)n;
  unsigned *ks = q, *vs = q + n, *kd = q + 2 * (size_t)n, *vd = q + 3 * (size_t)n;

  // (A) the keys of class c, the payloads and the class counts of the patch
  if (t < 8) ncls[t] = 0;
  __syncthreads();
  for (int i = t; i < n; i += 256) {
    const int p = base + i;
    const int y = a.labels[p];
    const bool in = !(a.loss_mask && !a.loss_mask[p]) && y < KM;
    float e = 0.f;
    if (in) {
      atomicAdd(&ncls[y], 1);
      if (a.logits) {
        float lg[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) lg[k] = a.logits[(size_t)p * KM + k];
        float mx = lg[0];
#pragma unroll
        for (int k = 1; k < KM; ++k) mx = lg[k] > mx ? lg[k] : mx;
        float se = 0.f, so = 0.f, exc = 0.f;
#pragma unroll
        for (int k = 0; k < KM; ++k) {
          const float ex = expf(lg[k] - mx);
          se += ex;
          if (k == c) exc = ex; else so += ex;
        }
        e = (y == c ? so : exc) / se;       // (1 - p_c as the sum of the others, never by subtraction)
      } else {
        e = a.err[(size_t)p * KM + c];
      }
    }
    if (a.logits) a.err[(size_t)p * KM + c] = e;
    ks[i] = in ? LOV_ONE - __float_as_uint(e) : 0xFFFFFFFFu;
    vs[i] = (unsigned)i | (in ? LOV_IN : 0u) | ((in && y == c) ? LOV_FG : 0u);
  }
  __syncthreads();
  int nb = 0, cb = 0;
#pragma unroll
  for (int k = 0; k < KM; ++k) { nb += ncls[k]; cb += ncls[k] > 0 ? 1 : 0; }
  const int N = ncls[c];
  const double f = nb ? (a.lam * (double)nb) / (double)cb : 0.0;
  if (c == 0 && t == 0) a.factor[b] = f;
  float g_in = 0.f, g_out = 0.f;
  if (a.dice) { g_in = a.dice[2 * (size_t)blockIdx.x]; g_out = a.dice[2 * (size_t)blockIdx.x + 1]; }

  if (N == 0) {                           // (the same for every thread) an absent class, or nothing in the loss: no order, no term
    for (int i = t; i < n; i += 256) {
      const unsigned v = vs[i];            // (written by this thread)
      const size_t o = (size_t)(base + i) * KM + c;
      a.grad[o] = (v & LOV_IN) ? (a.dice ? 0.f + g_out : 0.f) : 0.f;
      if (a.rank) a.rank[o] = 0xFFFFFFFFu;
    }
    if (t == 0) a.cls_loss[blockIdx.x] = 0.0;
    return;
  }

  // (B) the stable sort: wave w owns elements [w chunk, (w + 1) chunk)
  const int chunk = ((n + 255) >> 8) << 6;
  const int steps = chunk >> 6;
  for (int shift = 0; shift < 32; shift += 8) {
    for (int j = t; j < 1024; j += 256) (&hist[0][0])[j] = 0;
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
      const int i = wave * chunk + (s << 6) + lane;
      if (i < n) atomicAdd(&hist[wave][(ks[i] >> shift) & 255u], 1);
    }
    __syncthreads();
    {
      const int c0 = hist[0][t], c1 = hist[1][t], c2 = hist[2][t], c3 = hist[3][t];
      int total;
      const int ex = lov_block_prefix(((c0 + c1) + c2) + c3, lane, wave, wsum[(shift >> 3) & 1], total);      // (a barrier inside: every count is read)
      hist[0][t] = ex; hist[1][t] = ex + c0; hist[2][t] = ex + c0 + c1; hist[3][t] = ex + (c0 + c1) + c2;
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
      const int i = wave * chunk + (s << 6) + lane;
      const bool act = i < n;
      unsigned key = 0u, val = 0u;
      if (act) { key = ks[i]; val = vs[i]; }
      const unsigned d = (key >> shift) & 255u;
      unsigned long long peers = __ballot(act);            // ends as: the active lanes of this step with this lane's digit
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const bool one = ((d >> bit) & 1u) != 0u;
        const unsigned long long m = __ballot(act && one);
        peers &= one ? m : ~m;
      }
      const int below = __popcll(peers & ((1ull << lane) - 1ull));
      const int cnt = __popcll(peers);
      int pos = 0;
      if (act) pos = hist[wave][d] + below;
      __syncthreads();                     // (row `wave` of hist is this wave's alone; the barriers order its lanes' reads and writes)
      if (act && below == cnt - 1) hist[wave][d] = pos + 1;
      if (act) { kd[pos] = key; vd[pos] = val; }
      __syncthreads();
    }
    unsigned* tk = ks; ks = kd; kd = tk;
    unsigned* tv = vs; vs = vd; vd = tv;
  }

  // (C) in sorted order: F by a prefix count, the increment, the map, the ranks and the class's loss
  const int rounds = (n + 255) >> 8;
  int seen = 0;                           // foreground pixels in the rounds before this one
  double acc = 0.0;
  for (int r = 0; r < rounds; ++r) {
    const int i = (r << 8) + t;
    unsigned key = 0xFFFFFFFFu, val = 0u;
    if (i < n) { key = ks[i]; val = vs[i]; }
    const bool in = (val & LOV_IN) != 0u, fg = (val & LOV_FG) != 0u;
    int total;
    const int F = seen + lov_block_prefix(fg ? 1 : 0, lane, wave, wsum[r & 1], total);
    seen += total;
    if (i < n) {
      const size_t o = (size_t)(base + (int)(val & LOV_IDX)) * KM + c;
      float gv = 0.f;
      if (in) {
        const double U = (double)(N + (i - F));           // (i >= F and N >= 1: U >= 1)
        const double dJ = fg ? 1.0 / U : (double)(N - F) / (U * (U + 1.0));
        const float gf = (float)(f * dJ);
        gv = fg ? -gf : gf;
        if (a.dice) gv = gv + (fg ? g_in : g_out);
        acc += __dmul_rn((double)__uint_as_float(LOV_ONE - key), dJ);
      }
      a.grad[o] = gv;
      if (a.rank) a.rank[o] = in ? (unsigned)i : 0xFFFFFFFFu;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (t == 0) a.cls_loss[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// patch_loss[b] = (lam n_b / C_b) sum_c Loss_bc, the classes in ascending order (an absent class holds 0)
__global__ void __launch_bounds__(256) lovasz_patch_loss_kernel(const double* __restrict__ cls_loss, const double* __restrict__ factor,
                                                                int B, int K, double* __restrict__ patch_loss) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += cls_loss[(size_t)b * K + k];
  patch_loss[b] = factor[b] * s;
}

size_t lov_sums_bytes(long long B, int K) { return (size_t)(((B * K + B) * 8 + 15) / 16 * 16); }

template <int KM>
int lov_launch(int K, int B, hipStream_t st, const LovArgs& a) {
  if constexpr (KM < 8)
    if (K != KM) return lov_launch<KM + 1>(K, B, st, a);
  if (a.SS <= LOV_LDS_ELEMS) {
    static bool raised = false;              // above 64 KiB the dynamic LDS size has to be allowed once per kernel
    if (!raised) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_lovasz_kernel<KM, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)LOV_LDS_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        return DRS_ERR_HIP;
      }
      raised = true;
    }
    DRS_LAUNCH((patch_lovasz_kernel<KM, true>), dim3(B * KM), dim3(256), (size_t)a.SS * 16, st, a);
  } else {
    DRS_LAUNCH((patch_lovasz_kernel<KM, false>), dim3(B * KM), dim3(256), 0, st, a);
  }
  if (const int rc = DRS_LAUNCH_CHECK()) return rc;
  DRS_LAUNCH(lovasz_patch_loss_kernel, dim3((B + 255) / 256), dim3(256), 0, st, a.cls_loss, a.factor, B, K, a.patch_loss);
  return DRS_OK;
}

}  // namespace

extern "C" {

size_t drs_lovasz_scratch_bytes(int B, int S, int K) {
  if (B < 1 || S < 1 || (long long)B * S * S >= (1LL << 24) || K < 1 || K > 8) return 0;
  const long long SS = (long long)S * S;
  return lov_sums_bytes(B, K) + (SS > LOV_LDS_ELEMS ? (size_t)B * K * SS * 16 : 0);
}

int drs_patch_lovasz_grad(const float* logits, float* err, const unsigned char* labels, const unsigned char* loss_mask, int B, int S,
                          int K, double lam, const float* dice_coef, unsigned int* rank_out, float* grad_out, double* patch_loss_out,
                          void* scratch, size_t scratch_bytes, void* stream) {
  if (!err || !labels || !grad_out || !patch_loss_out) return DRS_ERR_ARG;
  if (B < 1 || S < 1 || (long long)B * S * S >= (1LL << 24) || K < 1 || K > 8) return DRS_ERR_ARG;
  if (!std::isfinite(lam) || !(lam > 0.0) || lam > 64.0) return DRS_ERR_ARG;
  if (!scratch || scratch_bytes < drs_lovasz_scratch_bytes(B, S, K) || (uintptr_t)scratch % 8) return DRS_ERR_ARG;
  if ((uintptr_t)dice_coef % 8) return DRS_ERR_ARG;
  LovArgs a;
  a.logits = logits; a.err = err; a.labels = labels; a.loss_mask = loss_mask; a.SS = S * S; a.lam = lam; a.dice = dice_coef;
  a.rank = rank_out; a.grad = grad_out; a.patch_loss = patch_loss_out;
  a.cls_loss = static_cast<double*>(scratch);
  a.factor = a.cls_loss + (size_t)B * K;
  a.pp = reinterpret_cast<unsigned*>(static_cast<char*>(scratch) + lov_sums_bytes(B, K));
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = lov_launch<1>(K, B, st, a)) return rc;
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
