// Local dense-CRF refinement of a whole-map class posterior (opt-in; include/drs.h: drs_crf_unary, drs_crf_step):
// mean-field iterations of a bilateral + smoothness Potts model over a (2R+1)^2 window dilated by `step`
// (Kraehenbuehl & Koltun 2011 in the local-window form of Teichmann & Cipolla 2018).  tests/crf_ref.py states the rule in fp64.
#include "drs_common.hpp"
#include "../../include/drs.h"
#include <float.h>
#include <cmath>

namespace {

constexpr int CRF_MAX_K = 8, CRF_MAX_C = 8, CRF_MAX_R = 6, CRF_MAX_STEP = 4, CRF_MAX_REACH = 12;
constexpr int CRF_TX = 32;            // output columns of a workgroup: half a wave per row, so a wave reads two LDS rows
constexpr int CRF_SLOTS = 16;         // rows of threads: 512 threads = two waves per SIMD
constexpr int CRF_P = 2;              // output pixels per thread, `step` rows apart: a staged neighbour serves both
constexpr int CRF_THREADS = CRF_TX * CRF_SLOTS;
constexpr int CRF_LDS_BYTES = 160 * 1024;
constexpr int CRF_TAB = 2 * CRF_MAX_R + 1;

// floats of one staged pixel record [Q_0 .. Q_K-1, f_0 .. f_C-1, pad]: 4 * odd, so that the 16-byte slots of the 16 lanes that one
// ds_read_b128 lane group serves (neighbouring pixels, record stride apart) fall on 16 different slots of the 64 banks
__host__ __device__ constexpr int crf_record(int K, int C) { return K + C <= 4 ? 4 : K + C <= 12 ? 12 : 20; }

// ---- unary: l = log softmax(beta u), Q0 = softmax(beta u), live = occur != 0 -----------------------------------------------------
// u is the score vector of DESIGN.md 8a.5 in fp32: the quotient sums / occur (logits) or the logarithm of that quotient clamped at
// FLT_MIN (probabilities); t = beta u is rounded to fp32 before the maximum is subtracted, as drs_stitch_finalize_scores_t forms it.
template <int K>
__global__ void crf_unary_kernel(const float* __restrict__ sums, const unsigned int* __restrict__ occur, size_t npix, int sums_are_prob,
                                 float beta, float* __restrict__ logp, float* __restrict__ q0, unsigned int* __restrict__ live) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned o = occur[i];
    const float ocf = (float)(o ? o : 1u);
    float t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float q = sums[i * K + k] / ocf;
      t[k] = __fmul_rn(beta, sums_are_prob ? logf(fmaxf(q, FLT_MIN)) : q);
    }
    float mx = t[0], se = 0.f, e[K];
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, t[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      t[k] = t[k] - mx;
      e[k] = expf(t[k]);
      se += e[k];
    }
    const float lse = logf(se);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      logp[i * K + k] = t[k] - lse;
      q0[i * K + k] = e[k] / se;
    }
    live[i] = o ? 1u : 0u;
  }
}

// ---- one mean-field iteration ----------------------------------------------------------------------------------------------------
struct CrfStepArgs {
  const float* q_in;
  const float* logp;
  const unsigned int* live;
  const void* tile;
  float* q_out;
  int tile_is_f64, h, w, row0, row_end, R, step, G;      // G: groups of CRF_P * step output rows per workgroup
  float cr;                                              // log2(e) / (2 theta_rgb^2)
  // per window offset (i + R, j + R): the appearance kernel's spatial factor w_app exp(-|d|^2 / (2 theta_xy^2)) and the whole
  // smoothness kernel w_smooth exp(-|d|^2 / (2 theta_s^2)), d = (i, j) * step; both 0 at the centre, which therefore adds nothing
  float app[CRF_TAB * CRF_TAB], smooth[CRF_TAB * CRF_TAB];
};

// the pair (p, q): kappa = app exp2(-cr |f_p - f_q|^2) + smooth, m_p += kappa Q_q.  One statement of the arithmetic for both of a
// thread's pixels, every product-sum an explicit fmaf: a pixel's bits do not depend on which slot of which workgroup computes it.
template <int K, int C, int S>
__device__ __forceinline__ void crf_pair(const float (&rec)[S], const float (&fp)[C], float app, float smooth, float cr, float (&m)[K]) {
  float d2 = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float d = fp[c] - rec[K + c];
    d2 = fmaf(d, d, d2);
  }
  const float kap = fmaf(app, __builtin_amdgcn_exp2f(-__fmul_rn(cr, d2)), smooth);
#pragma unroll
  for (int k = 0; k < K; ++k) m[k] = fmaf(kap, rec[k], m[k]);
}

// A workgroup owns CRF_TX columns x (CRF_P * step * G) rows of output pixels and stages their halo of reach R * step as pixel records
// in LDS: Q and the features of a neighbour that is inside the map and live, zeros otherwise -- a zero Q adds exactly nothing to the
// message (kappa is finite), so the window loop has no bounds or liveness test.  Thread (slot, lx) computes the pixels of column lx
// in rows r0 and r0 + step of the tile: neighbour row r0 + ii step is row i = ii of the first and i = ii - 1 of the second, so each
// record read from LDS serves two pairs, and every pixel still sums its window in the fixed order i ascending, then j ascending.
template <int K, int C>
__global__ void __launch_bounds__(CRF_THREADS) crf_step_kernel(const CrfStepArgs a) {
  constexpr int S = crf_record(K, C);
  extern __shared__ f32x4 crf_lds4[];
  float* lds = reinterpret_cast<float*>(crf_lds4);
  const int H = a.R * a.step;
  const int TY = CRF_P * a.step * a.G;
  const int LW = CRF_TX + 2 * H, LH = TY + 2 * H;
  const int x0 = blockIdx.x * CRF_TX, y0 = a.row0 + blockIdx.y * TY;
  const int tid = threadIdx.x;

  // (every load of a record is issued at once, from the nearest pixel of the map where the record lies outside it, and the record is
  // zeroed afterwards: a load that waited for the pixel's liveness would put two memory latencies in front of every record)
#pragma unroll 2
  for (int idx = tid; idx < LW * LH; idx += CRF_THREADS) {
    const int ry = idx / LW, rx = idx - ry * LW;
    const int gy = y0 - H + ry, gx = x0 - H + rx;
    const bool inside = gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
    const int cy = gy < 0 ? 0 : gy < a.h ? gy : a.h - 1, cx = gx < 0 ? 0 : gx < a.w ? gx : a.w - 1;
    const size_t p = (size_t)cy * a.w + cx;
    float rec[S];
#pragma unroll
    for (int e = 0; e < S; ++e) rec[e] = 0.f;
    const unsigned lv = a.live[p];
#pragma unroll
    for (int k = 0; k < K; ++k) rec[k] = a.q_in[p * K + k];
    if (a.tile_is_f64) {
#pragma unroll
      for (int c = 0; c < C; ++c) rec[K + c] = (float)static_cast<const double*>(a.tile)[p * C + c];
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) rec[K + c] = static_cast<const float*>(a.tile)[p * C + c];
    }
    if (!inside || !lv) {
#pragma unroll
      for (int e = 0; e < S; ++e) rec[e] = 0.f;
    }
    f32x4* dst = reinterpret_cast<f32x4*>(lds + (size_t)idx * S);
#pragma unroll
    for (int v = 0; v < S / 4; ++v) dst[v] = f32x4{rec[4 * v], rec[4 * v + 1], rec[4 * v + 2], rec[4 * v + 3]};
  }
  __syncthreads();

  const int slot = tid / CRF_TX, lx = tid - slot * CRF_TX;
  if (slot >= a.step * a.G) return;
  const int grp = slot / a.step;
  const int r0 = grp * (CRF_P * a.step) + (slot - grp * a.step);
  const int gx = x0 + lx;
  if (gx >= a.w) return;
  const int gy0 = y0 + r0, gy1 = gy0 + a.step;
  if (gy0 >= a.row_end) return;

  float fp0[C], fp1[C], m0[K], m1[K];
  {
    const float* c0 = lds + ((size_t)(r0 + H) * LW + lx + H) * S + K;
    const float* c1 = c0 + (size_t)a.step * LW * S;
#pragma unroll
    for (int c = 0; c < C; ++c) { fp0[c] = c0[c]; fp1[c] = c1[c]; }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) { m0[k] = 0.f; m1[k] = 0.f; }

  const int R = a.R;
  for (int ii = -R; ii <= R + 1; ++ii) {
    const float* row = lds + ((size_t)(r0 + H + ii * a.step) * LW + lx + H) * S;
    const bool on0 = ii <= R, on1 = ii > -R;                    // wave-uniform
    const int t0 = ((on0 ? ii : R) + R) * CRF_TAB + R, t1 = ((on1 ? ii - 1 : -R) + R) * CRF_TAB + R;      // table rows, kept in range
    for (int j = -R; j <= R; ++j) {
      const f32x4* src = reinterpret_cast<const f32x4*>(row + j * a.step * S);
      float rec[S];
#pragma unroll
      for (int v = 0; v < S / 4; ++v) {
        const f32x4 q = src[v];
        rec[4 * v] = q[0]; rec[4 * v + 1] = q[1]; rec[4 * v + 2] = q[2]; rec[4 * v + 3] = q[3];
      }
      if (on0) crf_pair<K, C, S>(rec, fp0, a.app[t0 + j], a.smooth[t0 + j], a.cr, m0);
      if (on1) crf_pair<K, C, S>(rec, fp1, a.app[t1 + j], a.smooth[t1 + j], a.cr, m1);
    }
  }

#pragma unroll
  for (int s = 0; s < CRF_P; ++s) {
    const int gy = s ? gy1 : gy0;
    if (gy >= a.row_end) break;
    const size_t p = (size_t)gy * a.w + gx;
    float* out = a.q_out + p * K;
    if (!a.live[p]) {                                           // a dead pixel keeps its Q
#pragma unroll
      for (int k = 0; k < K; ++k) out[k] = a.q_in[p * K + k];
      continue;
    }
    float z[K];
#pragma unroll
    for (int k = 0; k < K; ++k) z[k] = a.logp[p * K + k] + (s ? m1[k] : m0[k]);
    float mx = z[0], se = 0.f;
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, z[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      z[k] = expf(z[k] - mx);
      se += z[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = z[k] / se;
  }
}

// groups of CRF_P * step output rows per workgroup: as many as the thread rows carry, fewer where the halo would outgrow the LDS
int crf_groups(int K, int C, int R, int step) {
  const int H = R * step, S = crf_record(K, C);
  int G = CRF_SLOTS / step;
  while (G > 1 && (size_t)(CRF_P * step * G + 2 * H) * (CRF_TX + 2 * H) * S * 4 > (size_t)CRF_LDS_BYTES) --G;
  return G;
}

template <int K, int C>
int crf_launch(const CrfStepArgs& a, dim3 grid, size_t lds_bytes, hipStream_t stream) {
  static bool raised = false;              // above 64 KiB the dynamic LDS size has to be allowed once per kernel
  if (!raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&crf_step_kernel<K, C>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            CRF_LDS_BYTES) != hipSuccess) {
      (void)hipGetLastError();
      return DRS_ERR_HIP;
    }
    raised = true;
  }
  DRS_LAUNCH((crf_step_kernel<K, C>), grid, dim3(CRF_THREADS), lds_bytes, stream, a);
  return DRS_LAUNCH_CHECK();
}

template <int K>
int crf_launch_c(int C, const CrfStepArgs& a, dim3 grid, size_t lds_bytes, hipStream_t stream) {
  switch (C) {
    case 1: return crf_launch<K, 1>(a, grid, lds_bytes, stream);
    case 2: return crf_launch<K, 2>(a, grid, lds_bytes, stream);
    case 3: return crf_launch<K, 3>(a, grid, lds_bytes, stream);
    case 4: return crf_launch<K, 4>(a, grid, lds_bytes, stream);
    case 5: return crf_launch<K, 5>(a, grid, lds_bytes, stream);
    case 6: return crf_launch<K, 6>(a, grid, lds_bytes, stream);
    case 7: return crf_launch<K, 7>(a, grid, lds_bytes, stream);
    case 8: return crf_launch<K, 8>(a, grid, lds_bytes, stream);
  }
  return DRS_ERR_ARG;
}

bool crf_weight_ok(float v) { return std::isfinite(v) && v >= 0.f; }
bool crf_theta_ok(float v) { return std::isfinite(v) && v > 0.f; }

}  // namespace

extern "C" {

int drs_crf_unary(const float* sums, const unsigned int* occur, int h, int w, int K, int sums_are_prob, float beta, float* logp, float* q0,
                  unsigned int* live, void* stream) {
  if (!sums || !occur || !logp || !q0 || !live || h < 1 || w < 1 || K < 2 || K > CRF_MAX_K) return DRS_ERR_ARG;
  if (!(beta >= 1.0f / 64.0f && beta <= 64.0f)) return DRS_ERR_ARG;          // (a NaN fails both comparisons)
  const size_t n = (size_t)h * w;
  const size_t nb = (n + 255) / 256;
  const dim3 grid(nb < 4096 ? (unsigned)nb : 4096u);
  const int prob = sums_are_prob ? 1 : 0;
#define DRS_CRF_UNARY_CASE(KK) \
  case KK: DRS_LAUNCH(crf_unary_kernel<KK>, grid, dim3(256), 0, (hipStream_t)stream, sums, occur, n, prob, beta, logp, q0, live); break;
  switch (K) {
    DRS_CRF_UNARY_CASE(2) DRS_CRF_UNARY_CASE(3) DRS_CRF_UNARY_CASE(4) DRS_CRF_UNARY_CASE(5)
    DRS_CRF_UNARY_CASE(6) DRS_CRF_UNARY_CASE(7) DRS_CRF_UNARY_CASE(8)
  }
#undef DRS_CRF_UNARY_CASE
  return DRS_LAUNCH_CHECK();
}

int drs_crf_step(const float* q_in, const float* logp, const unsigned int* live, const void* tile, int tile_is_f64, int C, int h, int w,
                 int K, int row0, int rows, int R, int step, float w_app, float theta_xy, float theta_rgb, float w_smooth, float theta_s,
                 float* q_out, void* stream) {
  if (!q_in || !logp || !live || !tile || !q_out || q_in == q_out) return DRS_ERR_ARG;
  if (h < 1 || w < 1 || K < 2 || K > CRF_MAX_K || C < 1 || C > CRF_MAX_C) return DRS_ERR_ARG;
  if (row0 < 0 || rows < 1 || rows > h || row0 > h - rows) return DRS_ERR_ARG;
  if (R < 1 || R > CRF_MAX_R || step < 1 || step > CRF_MAX_STEP || R * step > CRF_MAX_REACH) return DRS_ERR_ARG;
  if (!crf_weight_ok(w_app) || !crf_weight_ok(w_smooth) || !crf_theta_ok(theta_xy) || !crf_theta_ok(theta_rgb) || !crf_theta_ok(theta_s))
    return DRS_ERR_ARG;
  CrfStepArgs a;
  a.q_in = q_in; a.logp = logp; a.live = live; a.tile = tile; a.q_out = q_out; a.tile_is_f64 = tile_is_f64 ? 1 : 0;
  a.h = h; a.w = w; a.row0 = row0; a.row_end = row0 + rows; a.R = R; a.step = step;
  a.G = crf_groups(K, C, R, step);
  a.cr = (float)(1.4426950408889634 / (2.0 * (double)theta_rgb * (double)theta_rgb));
  if (!std::isfinite(a.cr)) return DRS_ERR_ARG;          // a theta_rgb whose 1 / (2 theta^2) leaves fp32: cr * 0 would be a NaN
  for (int e = 0; e < CRF_TAB * CRF_TAB; ++e) a.app[e] = a.smooth[e] = 0.f;
  for (int i = -R; i <= R; ++i)
    for (int j = -R; j <= R; ++j) {
      if (i == 0 && j == 0) continue;
      const double d2 = (double)(i * i + j * j) * step * step;
      a.app[(i + R) * CRF_TAB + j + R] = (float)((double)w_app * exp(-d2 / (2.0 * (double)theta_xy * (double)theta_xy)));
      a.smooth[(i + R) * CRF_TAB + j + R] = (float)((double)w_smooth * exp(-d2 / (2.0 * (double)theta_s * (double)theta_s)));
    }
  const int H = R * step, TY = CRF_P * step * a.G;
  const size_t lds_bytes = (size_t)(TY + 2 * H) * (CRF_TX + 2 * H) * crf_record(K, C) * 4;
  if (lds_bytes > (size_t)CRF_LDS_BYTES) return DRS_ERR_ARG;
  const dim3 grid((w + CRF_TX - 1) / CRF_TX, (rows + TY - 1) / TY);
  if (grid.y > 65535u) return DRS_ERR_ARG;
  switch (K) {
    case 2: return crf_launch_c<2>(C, a, grid, lds_bytes, (hipStream_t)stream);
    case 3: return crf_launch_c<3>(C, a, grid, lds_bytes, (hipStream_t)stream);
    case 4: return crf_launch_c<4>(C, a, grid, lds_bytes, (hipStream_t)stream);
    case 5: return crf_launch_c<5>(C, a, grid, lds_bytes, (hipStream_t)stream);
    case 6: return crf_launch_c<6>(C, a, grid, lds_bytes, (hipStream_t)stream);
    case 7: return crf_launch_c<7>(C, a, grid, lds_bytes, (hipStream_t)stream);
    case 8: return crf_launch_c<8>(C, a, grid, lds_bytes, (hipStream_t)stream);
  }
  return DRS_ERR_ARG;
}

}  // extern "C"
