// The data-dependent pre-pass of the boundary (surface) loss of the training loss (opt-in; include/drs.h, "Training level: boundary
// (surface) loss"; tests/surface_loss_ref.py states the rule in numpy).  Kervadec et al., Boundary loss for highly
// unbalanced segmentation, MIDL 2019: the softmax probability of every class integrated against the class's signed distance map of
// the ground truth.  Its logit gradient is inv_n P_k (g_k - sum_c P_c g_c) with g = lam clamp(phi), which is what
// drs_classifier_loss_region adds for any per-(pixel, class) map, so the step runs the classifier once in its inference form, this
// pre-pass over the labels and the logits, and then the fused classifier with the map this pre-pass leaves.
//   per patch b and class c, over the COUNTED pixels of the patch (label < K, loss_mask set when given, valid set when given):
//     A = counted pixels with y = c, O = counted pixels with y != c; either empty: phi = 0 in the patch
//     D2(p) = min over the OTHER set of |p - q|^2  (exact integers; the patch's edge is no boundary)
//     phi   = +sqrt(D2) at p in O,  1 - sqrt(D2) at p in A           g_c(p) = (float)(lam clamp(phi, -clip, +clip))   (fp64, one rounding)
//     Loss_bc = sum_p g_c(p) P_c(p)   (fp64; P from the fp32 logits as the Lovasz keys form ex_c / se)
// One workgroup per (patch, class), which reads and writes its own patch only.  (A) the label / counted byte of every pixel; (B) one
// thread per column walks it down and up once and leaves, for both site sets at once, the distance to the nearest site of the column
// as uint16 (0xFFFF: none); (C) every thread takes pixels of the patch, lanes on consecutive x, and finds
// min_i (x - i)^2 + g[y][i]^2 along its row by scanning outward from x, four offsets to either side per round with their eight reads in
// flight together (one offset per round left the scan waiting on LDS latency: 0.180 -> 0.121 ms at 128 x 64 x 64, 0.370 -> 0.217 ms at
// 16 x 85 x 85, profiles/surface_loss/scan_ab.txt), until a round's first offset squared alone reaches the best so far: exact, parallel
// over all S^2 pixels, no dependent chain -- at patch sizes the S^3 bound costs less than one latency chain of a lower-envelope row
// pass with only S rows per workgroup.  The two planes and the bytes stay in LDS for S <= SURF_LDS_SIDE (5 S^2 bytes) and live in the
// caller's scratch above that.  The class's sum is a fixed-order block reduction; no floating-point atomics: a launch gives the same
// bits every time.  The classes' sums meet in a second, tiny launch.
#include "drs_common.hpp"
#include "../../include/drs.h"
#include <cmath>
#include <cstdint>

namespace {

constexpr int SURF_LDS_SIDE = 128;                    // 5 * 128^2 = 80 KiB of the 160 KiB a workgroup may take
constexpr unsigned SURF_NONE = 0xFFFFu;               // no site in the column
constexpr unsigned char SURF_OUT = 0xFFu;             // the byte of a pixel that is not in the loss
constexpr unsigned char SURF_LOSS_ONLY = 0x80u;       // + label: in the loss but not valid (not counted; the Dice part still applies)

struct SurfArgs {
  const float* logits;               // [B * SS][K] or null: no loss
  const unsigned char* labels;       // [B * SS]
  const unsigned char* loss_mask;    // [B * SS] or null
  const unsigned char* valid;        // [B * SS] or null
  int S, SS;
  double lam, clip;
  const float* dice;                 // [B][K][2] or null
  int accumulate;
  int* phi2;                         // [B * SS][K] or null
  float* grad;                       // [B * SS][K]
  double* cls_loss;                  // scratch [B][K]: Loss_bc
  double* patch_loss;                // [B]
  uint16_t* planes;                  // scratch [B K][plane]: the two column-distance planes of the form without LDS storage
  size_t plane_elems;                // uint16 per (patch, class) in `planes`
};

size_t surf_sums_bytes(long long B, int K) { return (size_t)((B * K * 8 + 15) / 16 * 16); }
size_t surf_plane_bytes(long long SS) { return (size_t)((SS * 4 + 15) / 16 * 16); }

template <int KM>
__device__ __forceinline__ unsigned char surf_code(const SurfArgs& a, int p) {
  const int y = a.labels[p];
  if (y >= KM || (a.loss_mask && !a.loss_mask[p])) return SURF_OUT;
  return (unsigned char)((a.valid && !a.valid[p]) ? (SURF_LOSS_ONLY | y) : y);
}

template <int KM, bool INLDS>
__global__ void __launch_bounds__(256) patch_surface_kernel(const SurfArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char surf_lds[];      // gA [SS] uint16, gO [SS] uint16, code [SS] when INLDS
  __shared__ int has[2];
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x / KM, c = blockIdx.x - b * KM;
  const int S = a.S, n = a.SS;
  const int base = b * n;                 // (B SS < 2^24: every pixel index fits an int)
  uint16_t* gA;
  unsigned char* code = nullptr;
  if constexpr (INLDS) { gA = reinterpret_cast<uint16_t*>(surf_lds); code = surf_lds + 4 * (size_t)n; }
  else gA = a.planes + (size_t)blockIdx.x * a.plane_elems;
  uint16_t* gO = gA + n;
  auto code_at = [&](int i) -> unsigned {
    if constexpr (INLDS) return code[i];
    else return surf_code<KM>(a, base + i);
  };

  // (A) the bytes, and whether the patch has a site of either kind
  if (t < 2) has[t] = 0;
  __syncthreads();
  {
    bool hA = false, hO = false;
    for (int i = t; i < n; i += 256) {
      const unsigned cd = surf_code<KM>(a, base + i);
      if constexpr (INLDS) code[i] = (unsigned char)cd;
      if (cd < 8u) { if ((int)cd == c) hA = true; else hO = true; }
    }
    if (hA) has[0] = 1;                   // (every writer stores the same value)
    if (hO) has[1] = 1;
  }
  __syncthreads();
  float g_in = 0.f, g_out = 0.f;
  if (a.dice) { g_in = a.dice[2 * (size_t)blockIdx.x]; g_out = a.dice[2 * (size_t)blockIdx.x + 1]; }

  if (!(has[0] && has[1])) {              // (the same for every thread) an absent class, a class without a contour, nothing counted: phi = 0
    for (int i = t; i < n; i += 256) {
      const unsigned cd = code_at(i);
      const size_t o = (size_t)(base + i) * KM + c;
      if (a.accumulate) {
        if (cd < 8u) a.grad[o] = a.grad[o] + 0.f;
      } else {
        a.grad[o] = (a.dice && cd != SURF_OUT) ? 0.f + ((int)(cd & 7u) == c ? g_in : g_out) : 0.f;
      }
      if (a.phi2) a.phi2[o] = 0;
    }
    if (t == 0) a.cls_loss[blockIdx.x] = 0.0;
    return;
  }

  // (B) column distances to the nearest site of either kind: down, then up
  for (int x = t; x < S; x += 256) {
    unsigned dA = SURF_NONE, dO = SURF_NONE;
    for (int y = 0; y < S; ++y) {
      const int i = y * S + x;
      const unsigned cd = code_at(i);
      if (cd < 8u) { if ((int)cd == c) dA = 0u; else dO = 0u; }
      gA[i] = (uint16_t)dA;
      gO[i] = (uint16_t)dO;
      if (dA != SURF_NONE) ++dA;            // (at most S - 1 < 4095)
      if (dO != SURF_NONE) ++dO;
    }
    dA = SURF_NONE; dO = SURF_NONE;
    for (int y = S - 1; y >= 0; --y) {
      const int i = y * S + x;
      const unsigned vA = gA[i], vO = gO[i];
      if (vA == 0u) dA = 0u;
      if (vO == 0u) dO = 0u;
      gA[i] = (uint16_t)(vA < dA ? vA : dA);
      gO[i] = (uint16_t)(vO < dO ? vO : dO);
      if (dA != SURF_NONE) ++dA;
      if (dO != SURF_NONE) ++dO;
    }
  }
  __syncthreads();

  // (C) the row scan, the map and the class's sum
  double acc = 0.0;
  for (int i = t; i < n; i += 256) {
    const unsigned cd = code_at(i);
    const int p = base + i;
    const size_t o = (size_t)p * KM + c;
    if (cd < 8u) {
      const int y = i / S, x = i - y * S;
      const bool inside = (int)cd == c;
      const uint16_t* row = (inside ? gO : gA) + y * S;
      unsigned v = row[x];
      int best = v == SURF_NONE ? 0x7FFFFFFF : (int)(v * v);
      const int dmax = x > S - 1 - x ? x : S - 1 - x;
      // four offsets to either side per round, their eight reads in flight together; a round whose first offset alone reaches the
      // best so far ends the scan (every candidate further out is at least that offset squared), the others only add candidates
      for (int d0 = 1; d0 <= dmax; d0 += 4) {
        if (d0 * d0 >= best) break;
        unsigned vl[4], vr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int d = d0 + j;
          vl[j] = x - d >= 0 ? (unsigned)row[x - d] : SURF_NONE;
          vr[j] = x + d < S ? (unsigned)row[x + d] : SURF_NONE;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int dd = (d0 + j) * (d0 + j);
          if (vl[j] != SURF_NONE) { const int cand = dd + (int)(vl[j] * vl[j]); best = cand < best ? cand : best; }
          if (vr[j] != SURF_NONE) { const int cand = dd + (int)(vr[j] * vr[j]); best = cand < best ? cand : best; }
        }
      }
      // (the other set is not empty: best <= 2 (S - 1)^2 < 2^26)
      const double sq = sqrt((double)best);
      double phi = inside ? 1.0 - sq : sq;
      if (a.clip > 0.0) phi = phi > a.clip ? a.clip : (phi < -a.clip ? -a.clip : phi);
      const float gf = (float)(a.lam * phi);
      if (a.logits) {
        float lg[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) lg[k] = a.logits[(size_t)p * KM + k];
        float mx = lg[0];
#pragma unroll
        for (int k = 1; k < KM; ++k) mx = lg[k] > mx ? lg[k] : mx;
        float se = 0.f, exc = 0.f;
#pragma unroll
        for (int k = 0; k < KM; ++k) {
          const float ex = expf(lg[k] - mx);
          se += ex;
          if (k == c) exc = ex;
        }
        acc += __dmul_rn((double)gf, (double)(exc / se));
      }
      if (a.accumulate) a.grad[o] = a.grad[o] + gf;
      else a.grad[o] = a.dice ? gf + (inside ? g_in : g_out) : gf;
      if (a.phi2) a.phi2[o] = inside ? -best : best;
    } else {
      if (!a.accumulate) a.grad[o] = (a.dice && cd != SURF_OUT) ? 0.f + ((int)(cd & 7u) == c ? g_in : g_out) : 0.f;
      if (a.phi2) a.phi2[o] = 0;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (t == 0) a.cls_loss[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// patch_loss[b] = sum_c Loss_bc, the classes in ascending order
__global__ void __launch_bounds__(256) surface_patch_loss_kernel(const double* __restrict__ cls_loss, int B, int K,
                                                                 double* __restrict__ patch_loss) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int k = 0; k < K; ++k) s += cls_loss[(size_t)b * K + k];
  patch_loss[b] = s;
}

template <int KM>
int surf_launch(int K, int B, hipStream_t st, const SurfArgs& a) {
  if constexpr (KM < 8)
    if (K != KM) return surf_launch<KM + 1>(K, B, st, a);
  if (a.S <= SURF_LDS_SIDE) {
    static bool raised = false;              // above 64 KiB the dynamic LDS size has to be allowed once per kernel
    if (!raised) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_surface_kernel<KM, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              5 * SURF_LDS_SIDE * SURF_LDS_SIDE) != hipSuccess) {
        (void)hipGetLastError();
        return DRS_ERR_HIP;
      }
      raised = true;
    }
    DRS_LAUNCH((patch_surface_kernel<KM, true>), dim3(B * KM), dim3(256), (size_t)a.SS * 5, st, a);
  } else {
    DRS_LAUNCH((patch_surface_kernel<KM, false>), dim3(B * KM), dim3(256), 0, st, a);
  }
  if (const int rc = DRS_LAUNCH_CHECK()) return rc;
  DRS_LAUNCH(surface_patch_loss_kernel, dim3((B + 255) / 256), dim3(256), 0, st, a.cls_loss, B, K, a.patch_loss);
  return DRS_OK;
}

}  // namespace

extern "C" {

size_t drs_surface_loss_scratch_bytes(int B, int S, int K) {
  if (B < 1 || S < 1 || (long long)B * S * S >= (1LL << 24) || K < 1 || K > 8) return 0;
  const long long SS = (long long)S * S;
  return surf_sums_bytes(B, K) + (S > SURF_LDS_SIDE ? (size_t)B * K * surf_plane_bytes(SS) : 0);
}

int drs_patch_surface_loss(const float* logits, const unsigned char* labels, const unsigned char* loss_mask,
                           const unsigned char* valid, int B, int S, int K, double lam, double clip, const float* dice_coef,
                           int accumulate, int* phi2_out, float* grad_io, double* patch_loss_out, void* scratch, size_t scratch_bytes,
                           void* stream) {
  if (!labels || !grad_io || !patch_loss_out) return DRS_ERR_ARG;
  if (B < 1 || S < 1 || (long long)B * S * S >= (1LL << 24) || K < 1 || K > 8) return DRS_ERR_ARG;
  if (!std::isfinite(lam) || !(lam > 0.0) || lam > 64.0) return DRS_ERR_ARG;
  if (!std::isfinite(clip) || !(clip == 0.0 || (clip >= 1.0 && clip <= 32768.0))) return DRS_ERR_ARG;
  if (dice_coef && accumulate) return DRS_ERR_ARG;
  if (!scratch || scratch_bytes < drs_surface_loss_scratch_bytes(B, S, K) || (uintptr_t)scratch % 8) return DRS_ERR_ARG;
  if ((uintptr_t)dice_coef % 8 || (uintptr_t)logits % 4 || (uintptr_t)grad_io % 4 || (uintptr_t)phi2_out % 4 ||
      (uintptr_t)patch_loss_out % 8)
    return DRS_ERR_ARG;
  SurfArgs a;
  a.logits = logits; a.labels = labels; a.loss_mask = loss_mask; a.valid = valid; a.S = S; a.SS = S * S; a.lam = lam; a.clip = clip;
  a.dice = dice_coef; a.accumulate = accumulate != 0; a.phi2 = phi2_out; a.grad = grad_io; a.patch_loss = patch_loss_out;
  a.cls_loss = static_cast<double*>(scratch);
  a.planes = reinterpret_cast<uint16_t*>(static_cast<char*>(scratch) + surf_sums_bytes(B, K));
  a.plane_elems = surf_plane_bytes((long long)S * S) / 2;
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = surf_launch<1>(K, B, st, a)) return rc;
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
