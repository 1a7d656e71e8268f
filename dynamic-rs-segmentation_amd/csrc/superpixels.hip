// Superpixels of a whole map and the vote of a label map inside regions (opt-in; include/drs.h: drs_superpixel_features,
// drs_superpixels, drs_region_vote).  tests/superpixel_ref.py states the rule in numpy.  After the byte features
// everything is integer and every cross-workgroup combination is an integer atomic add: every output is exact and independent of
// tiling and scheduling.
//
// SLIC (Achanta et al. 2012) on a grid of gh x gw centres, stated in integers:
//   sp_init_kernel     one thread per centre: the start position and its pixel's bytes; the centre's sums zeroed
//   sp_assign_kernel   one workgroup per 32 x 32 pixel tile: the centres of the tile's cells +- 1 staged in LDS (at most 11 x 11: a cell
//                      is at least 4 pixels wide), every pixel to the nearest of its up to nine candidates, the tile's sums per centre in
//                      LDS (a thread adds a run of pixels with one centre at once), one global atomic add per (centre, tile, word)
//   sp_update_kernel   (a LATER launch: the sums are final) one thread per centre: the rounded means, the count; the sums zeroed again
// The vote is K passes onto one 64-bit counter per region root: vote_add_kernel sums the weights of class k's pixels per root and tile
// in an LDS table and adds them at the root, vote_best_kernel keeps (sum, class) where it beats the best so far and zeroes the counter,
// vote_apply_kernel relabels.
// No workgroup waits for another anywhere.
#include "drs_common.hpp"
#include "../../include/drs.h"

namespace {

constexpr int SP_T = 32;                      // tile side
constexpr int SP_THREADS = 256;
constexpr int SP_RUN = 4;                     // consecutive pixels of a row per thread: 8 threads a tile row
constexpr int SP_MAX_C = 8;
constexpr int SP_CELLS = 11;                  // cells of a tile per axis: 32 / 4 + 1 touched, + 2 for the neighbours
constexpr int SP_MAX_SIDE = 32768;
constexpr int SP_MAX_K = 32;
constexpr int VT_HASH = 2 * SP_T * SP_T;    // slots of the vote's per-tile table
constexpr unsigned VT_APPLY_GRID = 2048;    // workgroups of the relabelling launch at most

// ------------------------------------------------------------------------------------------------------------------ features
struct FeatArgs {
  const void* tile;
  unsigned char* feat;
  long long n;                                // h w C
  int is_f64, C;
  float lo[SP_MAX_C], inv[SP_MAX_C];
};

__global__ void __launch_bounds__(SP_THREADS) sp_features_kernel(const FeatArgs a) {
  __shared__ float lo[SP_MAX_C], inv[SP_MAX_C];
  if (threadIdx.x < SP_MAX_C) { lo[threadIdx.x] = a.lo[threadIdx.x]; inv[threadIdx.x] = a.inv[threadIdx.x]; }
  __syncthreads();
  const long long e = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
  if (e >= a.n) return;
  const int c = (int)(e % a.C);
  const float v = a.is_f64 ? (float)((const double*)a.tile)[e] : ((const float*)a.tile)[e];
  const float t = __fmul_rn(__fsub_rn(v, lo[c]), inv[c]);      // two roundings: never one fma
  int q = 0;
  if (t > 0.0f) q = t >= 255.0f ? 255 : (int)rintf(t);          // !(t > 0) covers NaN
  a.feat[e] = (unsigned char)q;
}

// ------------------------------------------------------------------------------------------------------------------ SLIC
struct SpArgs {
  const unsigned char* feat;
  int* assign;
  unsigned char* colour;
  int* centres;                               // [gh gw][C + 3]: cx, cy, f.., n
  unsigned int* sums;                         // the scratch, [gh gw][C + 3]: sum x, sum y, sum f.., n
  int h, w, gh, gw, tiles_x;
  unsigned int S2, m2;
};

__device__ __forceinline__ int sp_cell(int x, int g, int w) {
  const int c = x * g / w;                    // x < 2^15, g <= 2^13
  return c < g - 1 ? c : g - 1;
}

template <int C>
__global__ void __launch_bounds__(SP_THREADS) sp_init_kernel(const SpArgs a) {
  const int id = blockIdx.x * SP_THREADS + threadIdx.x;
  if (id >= a.gh * a.gw) return;
  const int cj = id / a.gw, ci = id - cj * a.gw;
  const int cx = (2 * ci + 1) * a.w / (2 * a.gw), cy = (2 * cj + 1) * a.h / (2 * a.gh);
  int* ctr = a.centres + (size_t)id * (C + 3);
  unsigned int* sum = a.sums + (size_t)id * (C + 3);
  const unsigned char* f = a.feat + ((size_t)cy * a.w + cx) * C;
  ctr[0] = cx;
  ctr[1] = cy;
#pragma unroll
  for (int c = 0; c < C; ++c) ctr[2 + c] = f[c];
  ctr[C + 2] = 0;
#pragma unroll
  for (int k = 0; k < C + 3; ++k) sum[k] = 0u;
}

template <int C>
__global__ void __launch_bounds__(SP_THREADS) sp_assign_kernel(const SpArgs a) {
  __shared__ int lc[SP_CELLS * SP_CELLS][C + 2];
  __shared__ unsigned int acc[SP_CELLS * SP_CELLS][C + 3];
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * SP_T, x0 = tx * SP_T;
  const int x1 = x0 + SP_T - 1 < a.w ? x0 + SP_T - 1 : a.w - 1, y1 = y0 + SP_T - 1 < a.h ? y0 + SP_T - 1 : a.h - 1;
  int ci_lo = sp_cell(x0, a.gw, a.w) - 1, ci_hi = sp_cell(x1, a.gw, a.w) + 1;
  int cj_lo = sp_cell(y0, a.gh, a.h) - 1, cj_hi = sp_cell(y1, a.gh, a.h) + 1;
  ci_lo = ci_lo < 0 ? 0 : ci_lo;
  cj_lo = cj_lo < 0 ? 0 : cj_lo;
  ci_hi = ci_hi > a.gw - 1 ? a.gw - 1 : ci_hi;
  cj_hi = cj_hi > a.gh - 1 ? a.gh - 1 : cj_hi;
  const int ncx = ci_hi - ci_lo + 1, ncells = ncx * (cj_hi - cj_lo + 1);      // at most SP_CELLS each way: a cell is >= 4 pixels wide
  for (int l = threadIdx.x; l < ncells; l += SP_THREADS) {
    const int j = l / ncx, i = l - j * ncx;
    const int* ctr = a.centres + (size_t)((cj_lo + j) * a.gw + ci_lo + i) * (C + 3);
#pragma unroll
    for (int k = 0; k < C + 2; ++k) lc[l][k] = ctr[k];
#pragma unroll
    for (int k = 0; k < C + 3; ++k) acc[l][k] = 0u;
  }
  __syncthreads();

  const int y = y0 + (int)(threadIdx.x >> 3), xq = x0 + (int)(threadIdx.x & 7) * SP_RUN;
  if (y < a.h && xq < a.w) {
    const int cj = sp_cell(y, a.gh, a.h);
    int run = -1;                             // the tile-local centre the sums below belong to
    unsigned int rx = 0u, ry = 0u, rn = 0u, rf[C];
    auto flush = [&]() {
      if (run < 0) return;
      atomicAdd(&acc[run][0], rx);
      atomicAdd(&acc[run][1], ry);
#pragma unroll
      for (int c = 0; c < C; ++c) atomicAdd(&acc[run][2 + c], rf[c]);
      atomicAdd(&acc[run][C + 2], rn);
    };
    for (int q = 0; q < SP_RUN; ++q) {
      const int x = xq + q;
      if (x >= a.w) break;
      const size_t p = (size_t)y * a.w + x;
      int f[C];
#pragma unroll
      for (int c = 0; c < C; ++c) f[c] = a.feat[p * C + c];
      const int ci = sp_cell(x, a.gw, a.w);
      // candidates in ascending id, strict <: ties go to the lower id.  The key is below 2^32 (include/drs.h).
      unsigned int best = 0xffffffffu;
      int bl = 0, bi = 0, bj = 0;
      for (int dj = -1; dj <= 1; ++dj) {
        const int jj = cj + dj;
        if (jj < 0 || jj >= a.gh) continue;
        for (int di = -1; di <= 1; ++di) {
          const int ii = ci + di;
          if (ii < 0 || ii >= a.gw) continue;
          const int l = (jj - cj_lo) * ncx + (ii - ci_lo);
          const int dx = x - lc[l][0], dy = y - lc[l][1];
          unsigned int dc = 0u;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const int d = f[c] - lc[l][2 + c];
            dc += (unsigned int)(d * d);
          }
          const unsigned int key = a.S2 * dc + a.m2 * (unsigned int)(dx * dx + dy * dy);
          if (key < best) { best = key; bl = l; bi = ii; bj = jj; }
        }
      }
      a.assign[p] = bj * a.gw + bi;
      a.colour[p] = (unsigned char)((bj & 3) * 4 + (bi & 3));
      if (bl != run) {
        flush();
        run = bl;
        rx = ry = rn = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c) rf[c] = 0u;
      }
      rx += (unsigned int)x;
      ry += (unsigned int)y;
      rn += 1u;
#pragma unroll
      for (int c = 0; c < C; ++c) rf[c] += (unsigned int)f[c];
    }
    flush();
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ncells * (C + 3); e += SP_THREADS) {
    const int l = e / (C + 3), k = e - l * (C + 3);
    const unsigned int v = acc[l][k];
    if (!v) continue;
    const int j = l / ncx, i = l - j * ncx;
    atomicAdd(a.sums + (size_t)((cj_lo + j) * a.gw + ci_lo + i) * (C + 3) + k, v);
  }
}

// a centre without pixels keeps its values; n is stored either way
template <int C>
__global__ void __launch_bounds__(SP_THREADS) sp_update_kernel(const SpArgs a) {
  const int id = blockIdx.x * SP_THREADS + threadIdx.x;
  if (id >= a.gh * a.gw) return;
  int* ctr = a.centres + (size_t)id * (C + 3);
  unsigned int* sum = a.sums + (size_t)id * (C + 3);
  const unsigned long long n = sum[C + 2];
  if (n) {
#pragma unroll
    for (int k = 0; k < C + 2; ++k) ctr[k] = (int)((2ull * sum[k] + n) / (2ull * n));
  }
  ctr[C + 2] = (int)n;
#pragma unroll
  for (int k = 0; k < C + 3; ++k) sum[k] = 0u;
}

template <int C>
int sp_run(const SpArgs& a, int iters, hipStream_t st) {
  const unsigned cblocks = (unsigned)((a.gh * a.gw + SP_THREADS - 1) / SP_THREADS);
  const unsigned ntiles = (unsigned)a.tiles_x * (unsigned)((a.h + SP_T - 1) / SP_T);
  DRS_LAUNCH(sp_init_kernel<C>, dim3(cblocks), dim3(SP_THREADS), 0, st, a);
  int rc = DRS_LAUNCH_CHECK();
  for (int it = 0; it < iters && rc == DRS_OK; ++it) {
    DRS_LAUNCH(sp_assign_kernel<C>, dim3(ntiles), dim3(SP_THREADS), 0, st, a);
    rc = DRS_LAUNCH_CHECK();
    if (rc != DRS_OK) break;
    DRS_LAUNCH(sp_update_kernel<C>, dim3(cblocks), dim3(SP_THREADS), 0, st, a);
    rc = DRS_LAUNCH_CHECK();
  }
  return rc;
}

bool sp_shape_ok(int h, int w) { return h >= 1 && w >= 1 && h <= SP_MAX_SIDE && w <= SP_MAX_SIDE; }

int sp_grid(int side, int S) { return side / S > 1 ? side / S : 1; }

// ------------------------------------------------------------------------------------------------------------------ the vote
struct VoteArgs {
  const unsigned char* in;
  unsigned char* out;
  const int* label;
  const unsigned char* weight;
  unsigned long long* sum;                    // scratch [h w]: the weight of the class of the pass, at the region's root
  unsigned long long* best;                   // scratch [h w]: (largest sum so far << 8) | (255 - its class), at the root; 0 = none
  unsigned int* counters;
  int n, K, h, w, tiles_x;
};

__global__ void __launch_bounds__(SP_THREADS) vote_init_kernel(const VoteArgs a) {
  const int p = blockIdx.x * SP_THREADS + threadIdx.x;
  if (p < 2) a.counters[p] = 0u;
  if (p < a.n && a.label[p] == p) { a.sum[p] = 0ull; a.best[p] = 0ull; }
}

// the per-tile (root -> weight) table: at most 1024 distinct roots in VT_HASH slots, so a probe ends; a tile's sum is below 2^18
__device__ __forceinline__ void vote_count(int* key, unsigned int* cnt, int root, unsigned int c) {
  unsigned int s = ((unsigned int)root * 2654435761u) >> 21;             // 11 bits: VT_HASH slots
  for (;;) {
    const int old = atomicCAS(key + s, -1, root);
    if (old == -1 || old == root) break;
    s = (s + 1) & (VT_HASH - 1);
  }
  atomicAdd(cnt + s, c);
}

// one workgroup per 32 x 32 tile; a thread walks SP_RUN consecutive pixels of a row and adds a run of one root at once; the tile's sums
// per root in LDS, one global atomic add per (region, tile)
__global__ void __launch_bounds__(SP_THREADS) vote_add_kernel(const VoteArgs a, int k) {
  __shared__ int key[VT_HASH];
  __shared__ unsigned int cnt[VT_HASH];
  for (int s = threadIdx.x; s < VT_HASH; s += SP_THREADS) { key[s] = -1; cnt[s] = 0u; }
  __syncthreads();
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y = ty * SP_T + (int)(threadIdx.x >> 3), xq = tx * SP_T + (int)(threadIdx.x & 7) * SP_RUN;
  if (y < a.h && xq < a.w) {
    int run = -1;
    unsigned int rs = 0u;
    for (int q = 0; q < SP_RUN && xq + q < a.w; ++q) {
      const int p = y * a.w + xq + q;
      int r = -1;
      unsigned int wv = 0u;
      if (a.in[p] == k) {
        r = a.label[p];
        wv = a.weight ? a.weight[p] : 1u;
      }
      if (r != run) {
        if (run >= 0 && rs) vote_count(key, cnt, run, rs);
        run = r;
        rs = 0u;
      }
      rs += wv;
    }
    if (run >= 0 && rs) vote_count(key, cnt, run, rs);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < VT_HASH; s += SP_THREADS)
    if (key[s] >= 0) atomicAdd(a.sum + key[s], (unsigned long long)cnt[s]);
}

// (a LATER launch: the sums of class k are final)  Classes come in ascending order and only a larger sum replaces: ties to the lower class.
__global__ void __launch_bounds__(SP_THREADS) vote_best_kernel(const VoteArgs a, int k) {
  const int p = blockIdx.x * SP_THREADS + threadIdx.x;
  if (p >= a.n || a.label[p] != p) return;
  const unsigned long long v = a.sum[p];
  if (!v) return;
  const unsigned long long cand = (v << 8) | (unsigned long long)(255 - k);       // v < 2^38
  if (cand > a.best[p]) a.best[p] = cand;
  a.sum[p] = 0ull;
}

// every pixel is read and written by one thread only, so out == in is fine.  A bounded grid walks the map: the two counts are kept in
// registers, combined per wavefront and per workgroup, and reach the counters with one atomic add per workgroup
__global__ void __launch_bounds__(SP_THREADS) vote_apply_kernel(const VoteArgs a) {
  __shared__ unsigned int tally[2];
  if (threadIdx.x < 2) tally[threadIdx.x] = 0u;
  __syncthreads();
  unsigned int roots = 0u, changed = 0u;
  for (long long q = (long long)blockIdx.x * SP_THREADS + threadIdx.x; q < a.n; q += (long long)gridDim.x * SP_THREADS) {
    const int p = (int)q;
    const int b = a.in[p], r = a.label[p];
    int nb = b;
    if (b < a.K) {
      const unsigned long long best = a.best[r];
      if (best) nb = 255 - (int)(best & 255ull);
    }
    a.out[p] = (unsigned char)nb;
    roots += r == p ? 1u : 0u;
    changed += nb != b ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    roots += __shfl_xor(roots, off);
    changed += __shfl_xor(changed, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&tally[0], roots);
    atomicAdd(&tally[1], changed);
  }
  __syncthreads();
  if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(a.counters + threadIdx.x, tally[threadIdx.x]);
}

}  // namespace

extern "C" {

int drs_superpixel_features(const void* tile, int tile_is_f64, int C, int h, int w, const float* lo, const float* inv, unsigned char* feat,
                            void* stream) {
  if (!tile || !lo || !inv || !feat || C < 1 || C > SP_MAX_C || !sp_shape_ok(h, w) || (tile_is_f64 != 0 && tile_is_f64 != 1))
    return DRS_ERR_ARG;
  FeatArgs a = {};
  a.tile = tile;
  a.feat = feat;
  a.n = (long long)h * w * C;
  a.is_f64 = tile_is_f64;
  a.C = C;
  for (int c = 0; c < C; ++c) { a.lo[c] = lo[c]; a.inv[c] = inv[c]; }
  DRS_LAUNCH(sp_features_kernel, dim3((unsigned)((a.n + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

size_t drs_superpixel_scratch_bytes(int C, int h, int w, int S) {
  if (C < 1 || C > SP_MAX_C || !sp_shape_ok(h, w) || S < 4 || S > 32) return 0;
  return (size_t)sp_grid(h, S) * (size_t)sp_grid(w, S) * (size_t)(C + 3) * sizeof(unsigned int);
}

int drs_superpixels(const unsigned char* feat, int C, int h, int w, int S, int m, int iters, int* assign, unsigned char* colour,
                    int* centres, void* scratch, void* stream) {
  if (!feat || !assign || !colour || !centres || !scratch || C < 1 || C > SP_MAX_C || !sp_shape_ok(h, w) || S < 4 || S > 32 || m < 1 ||
      m > 40 || iters < 1 || iters > 16)
    return DRS_ERR_ARG;
  const SpArgs a = {feat, assign, colour, centres, (unsigned int*)scratch, h, w, sp_grid(h, S), sp_grid(w, S), (w + SP_T - 1) / SP_T,
                    (unsigned int)(S * S), (unsigned int)(m * m)};
  hipStream_t st = (hipStream_t)stream;
  switch (C) {
    case 1: return sp_run<1>(a, iters, st);
    case 2: return sp_run<2>(a, iters, st);
    case 3: return sp_run<3>(a, iters, st);
    case 4: return sp_run<4>(a, iters, st);
    case 5: return sp_run<5>(a, iters, st);
    case 6: return sp_run<6>(a, iters, st);
    case 7: return sp_run<7>(a, iters, st);
    default: return sp_run<8>(a, iters, st);
  }
}

size_t drs_region_vote_scratch_bytes(int h, int w) { return sp_shape_ok(h, w) ? (size_t)h * (size_t)w * 16 : 0; }

int drs_region_vote(const unsigned char* map_in, const int* label, const unsigned char* weight, int h, int w, int K, void* scratch,
                    unsigned char* map_out, unsigned int* counters, void* stream) {
  if (!map_in || !label || !scratch || !map_out || !counters || !sp_shape_ok(h, w) || K < 1 || K > SP_MAX_K) return DRS_ERR_ARG;
  const int n = h * w;                        // at most 2^30
  unsigned long long* words = (unsigned long long*)scratch;
  const VoteArgs a = {map_in, map_out, label, weight, words, words + n, counters, n, K, h, w, (w + SP_T - 1) / SP_T};
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n + SP_THREADS - 1) / SP_THREADS);
  const unsigned ntiles = (unsigned)a.tiles_x * (unsigned)((h + SP_T - 1) / SP_T);
  DRS_LAUNCH(vote_init_kernel, dim3(blocks), dim3(SP_THREADS), 0, st, a);
  int rc = DRS_LAUNCH_CHECK();
  for (int k = 0; k < K && rc == DRS_OK; ++k) {
    DRS_LAUNCH(vote_add_kernel, dim3(ntiles), dim3(SP_THREADS), 0, st, a, k);
    rc = DRS_LAUNCH_CHECK();
    if (rc != DRS_OK) break;
    DRS_LAUNCH(vote_best_kernel, dim3(blocks), dim3(SP_THREADS), 0, st, a, k);
    rc = DRS_LAUNCH_CHECK();
  }
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(vote_apply_kernel, dim3(blocks < VT_APPLY_GRID ? blocks : VT_APPLY_GRID), dim3(SP_THREADS), 0, st, a);
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
