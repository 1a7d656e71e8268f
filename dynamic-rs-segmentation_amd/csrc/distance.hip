// Exact, unbounded squared Euclidean distance transform of a byte map, and the surface-distance table of a (truth, prediction) pair of
// label maps on top of it (opt-in; include/drs.h: drs_distance_transform, drs_surface_histogram).  HD95, ASSD and the
// normalised surface Dice are sums over that table (metrics.surface_scores).  tests/surface_ref.py states the rule in numpy.
// Everything is integer arithmetic; the two square roots of the table are fixed up to the exact integer.
//
// The transform is separable (Meijster, Roerdink, Hesselink, A general algorithm for computing distance transforms in linear time,
// 2000), three launches:
//   1a  dt_strip_ends_kernel   a thread per (strip of 64 rows, column): g = 0 at a site, NONE elsewhere; the strip's first and last site row
//   1b  dt_columns_kernel      a thread per (strip, column): the nearest site above / below the strip from the strips' ends, then one
//                              sweep down and one up inside the strip: g[y][x] = the distance along the column to its nearest site
//   2   dt_rows_kernel         a wave per 16 rows, a lane per row: the lower envelope of the parabolas (x - i)^2 + g[y][i]^2 along the
//                              row, stack in scratch interleaved by row (entry q of row y at [q h + y]: lanes stay unit-stride) with
//                              its top mirrored in LDS, then the fill from the right.  g is read and d2 written through a 16 x 256
//                              LDS tile, so that every global access has its 64 lanes on consecutive x.
// In all of them lanes sit on the unit-stride axis.  A column without a site never enters the envelope: it is skipped.
// Up to two transforms share a launch (grid z / y): the table's two directions of one class.
#include "drs_common.hpp"
#include "../../include/drs.h"
#include <cmath>

namespace {

constexpr int DT_STRIP = 64;                // rows of a column strip of phase 1
constexpr int DT_LANES = 64;                // threads of a phase-2 workgroup: one wave
constexpr int DT_TW = 256;                  // columns of the LDS tile of phase 2: four per lane
constexpr int DT_ROWS = 16;                 // rows of a phase-2 workgroup
constexpr int DT_WIN = 16;                  // stack entries per row mirrored in LDS (a power of two)
constexpr int DT_COLS = 256;                // threads (columns) of a phase-1 workgroup
constexpr unsigned int DT_NONE = 0xFFFFu;   // g of a column without a site; a real g is at most 32767
constexpr int DT_MAX_SIDE = 32768;
constexpr long long DT_MAX_PIX = 1LL << 28;
constexpr int DT_BATCH = 2;
constexpr int SF_MAX_K = 8;
constexpr int SF_BINS = DRS_SURFACE_BINS;
constexpr int SF_THREADS = 256;
constexpr int SF_MAX_GRID = 2048;           // persistent workgroups of the pixel kernels: each sees at most 2^28 / 2048 pixels

// Where the sites of one transform come from.  The byte at p is veil_label where veil[p] == veil_label, else map[p].  With `edge`
// (the table's path: edge[p] = "some 4-neighbour inside the map carries another byte", made once for all classes) a site is a pixel of
// byte cls with edge set; without it the mode decides.
struct DtSrc {
  const unsigned char* map;
  const unsigned char* veil;
  const unsigned char* edge;
  int veil_label, mode, cls;
};

struct DtArgs {
  DtSrc src[DT_BATCH];
  int h, w, nstrips;
  const unsigned int* cnt;                  // null, or the table's contour counts [2][8]: the launch runs iff both sets of cnt_cls are non-empty
  int cnt_cls;
  unsigned short* g;                        // [batch][h][w]
  int* first;                               // [batch][nstrips][w]
  int* last;
  unsigned long long* stack;                // [batch][w][h]
  unsigned int* d2[DT_BATCH];
};

__device__ __forceinline__ bool dt_active(const DtArgs& a) {
  return !a.cnt || (a.cnt[a.cnt_cls] != 0u && a.cnt[SF_MAX_K + a.cnt_cls] != 0u);
}

__device__ __forceinline__ int dt_byte(const DtSrc& s, size_t i) {
  return (s.veil && s.veil[i] == s.veil_label) ? s.veil_label : s.map[i];
}

__device__ __forceinline__ bool dt_site(const DtSrc& s, int y, int x, int h, int w) {
  const size_t i = (size_t)y * w + x;
  const int b = dt_byte(s, i);
  if (s.edge) return b == s.cls && s.edge[i] != 0;
  if (s.mode == DRS_DT_CLASS) return b == s.cls;
  if (s.mode == DRS_DT_NOT_CLASS) return b != s.cls;
  if (b != s.cls) return false;
  return (y > 0 && dt_byte(s, i - w) != b) || (y + 1 < h && dt_byte(s, i + w) != b) || (x > 0 && dt_byte(s, i - 1) != b) ||
         (x + 1 < w && dt_byte(s, i + 1) != b);
}

__global__ void __launch_bounds__(DT_COLS) dt_strip_ends_kernel(const DtArgs a) {
  if (!dt_active(a)) return;
  const int x = blockIdx.x * DT_COLS + threadIdx.x;
  if (x >= a.w) return;
  const int s = blockIdx.y, b = blockIdx.z;
  const DtSrc src = b ? a.src[1] : a.src[0];
  const size_t n = (size_t)a.h * a.w;
  unsigned short* g = a.g + (size_t)b * n;
  const int y0 = s * DT_STRIP, y1 = y0 + DT_STRIP < a.h ? y0 + DT_STRIP : a.h;
  int fi = -1, la = -1;
  for (int y = y0; y < y1; ++y) {
    const bool site = dt_site(src, y, x, a.h, a.w);
    g[(size_t)y * a.w + x] = site ? (unsigned short)0 : (unsigned short)DT_NONE;
    if (site) {
      if (fi < 0) fi = y;
      la = y;
    }
  }
  const size_t e = ((size_t)b * a.nstrips + s) * a.w + x;
  a.first[e] = fi;
  a.last[e] = la;
}

__global__ void __launch_bounds__(DT_COLS) dt_columns_kernel(const DtArgs a) {
  if (!dt_active(a)) return;
  const int x = blockIdx.x * DT_COLS + threadIdx.x;
  if (x >= a.w) return;
  const int s = blockIdx.y, b = blockIdx.z;
  const size_t n = (size_t)a.h * a.w;
  unsigned short* g = a.g + (size_t)b * n;
  const int* first = a.first + (size_t)b * a.nstrips * a.w + x;
  const int* last = a.last + (size_t)b * a.nstrips * a.w + x;
  int above = -1, below = -1;
  for (int sp = s - 1; sp >= 0 && above < 0; --sp) above = last[(size_t)sp * a.w];
  for (int sp = s + 1; sp < a.nstrips && below < 0; ++sp) below = first[(size_t)sp * a.w];
  const int y0 = s * DT_STRIP, y1 = y0 + DT_STRIP < a.h ? y0 + DT_STRIP : a.h;
  int cur = above;
  for (int y = y0; y < y1; ++y) {
    const size_t i = (size_t)y * a.w + x;
    if (g[i] == 0) cur = y;
    g[i] = cur >= 0 ? (unsigned short)(y - cur) : (unsigned short)DT_NONE;
  }
  cur = below;
  for (int y = y1 - 1; y >= y0; --y) {
    const size_t i = (size_t)y * a.w + x;
    const int v = g[i];
    if (v == 0) cur = y;
    if (cur >= 0 && cur - y < v) g[i] = (unsigned short)(cur - y);
  }
}

// one stack entry: the parabola's column s, the first column t at which it is the lowest, and its g: 15 bits each
__device__ __forceinline__ unsigned long long dt_pack(int s, int t, unsigned int g) {
  return (unsigned long long)s | ((unsigned long long)t << 16) | ((unsigned long long)g << 32);
}
__device__ __forceinline__ void dt_unpack(unsigned long long e, int& s, int& t, unsigned int& g) {
  s = (int)(e & 0xFFFFu);
  t = (int)((e >> 16) & 0xFFFFu);
  g = (unsigned int)(e >> 32);
}
// (x - i)^2 + g^2: |x - i| and g are below 2^15, so both squares are 24-bit multiplies (full rate) and the sum stays below 2^31
__device__ __forceinline__ unsigned int dt_f(int x, int i, unsigned int gi) {
  const int d = x - i;
  return (unsigned int)__mul24(d, d) + __umul24(gi, gi);
}

// A wave per DT_ROWS rows, lanes 0 .. DT_ROWS - 1 on one row each in the two sequential passes (a row is a chain of dependent steps:
// what hides its latency is the number of waves, so a wave takes few rows), all 64 lanes on consecutive columns where g is read and d2
// written.  The stack lives in scratch; its top DT_WIN entries per row are mirrored in LDS, refilled DT_WIN at a time (independent
// loads, one latency) when the pops run below the mirror: slot k % DT_WIN holds entry k for every k in [lo, q].
__global__ void __launch_bounds__(DT_LANES) dt_rows_kernel(const DtArgs a) {
  if (!dt_active(a)) return;
  __shared__ unsigned int tile[DT_ROWS][DT_TW + 1];
  __shared__ unsigned long long win[DT_WIN][DT_ROWS];
  const int lane = threadIdx.x, b = blockIdx.y;
  const int h = a.h, w = a.w;
  const int y0 = blockIdx.x * DT_ROWS, y = y0 + lane;
  const bool live = lane < DT_ROWS && y < h;
  const int row = live ? lane : 0;
  const size_t n = (size_t)h * w;
  const unsigned short* g = a.g + (size_t)b * n;
  unsigned long long* st = a.stack + (size_t)b * n + (live ? y : 0);      // entry q of this row: st[q h]
  unsigned int* out = b ? a.d2[1] : a.d2[0];
  int q = -1, lo = 0, ts = 0, tt = 0;       // the top of the stack is kept in registers as well
  unsigned int tg = 0;
  auto push = [&](int s, int t, unsigned int gs) {
    ++q; ts = s; tt = t; tg = gs;
    const unsigned long long e = dt_pack(s, t, gs);
    st[(size_t)q * h] = e;
    win[q & (DT_WIN - 1)][row] = e;
    if (q - DT_WIN + 1 > lo) lo = q - DT_WIN + 1;
  };
  auto pop = [&]() {
    --q;
    if (q < 0) return;
    if (q < lo) {
      lo = q - DT_WIN + 1 > 0 ? q - DT_WIN + 1 : 0;
#pragma unroll
      for (int i = 0; i < DT_WIN; ++i) {
        const int k = q - i > lo ? q - i : lo;          // (clamped, not skipped: entry lo may be copied again, and no load sits in a branch)
        win[k & (DT_WIN - 1)][row] = st[(size_t)k * h];
      }
    }
    dt_unpack(win[q & (DT_WIN - 1)][row], ts, tt, tg);
  };
  for (int x0 = 0; x0 < w; x0 += DT_TW) {
    // (the addresses are clamped into the map and the value chosen afterwards: no branch around a load, so all of them are in flight
    // at once and the wave waits for memory once per tile)
    unsigned short v[DT_ROWS][DT_TW / DT_LANES];
#pragma unroll
    for (int r = 0; r < DT_ROWS; ++r) {
#pragma unroll
      for (int c = 0; c < DT_TW / DT_LANES; ++c) {
        const int yy = y0 + r, xx = x0 + c * DT_LANES + lane;
        v[r][c] = g[(size_t)(yy < h ? yy : h - 1) * w + (xx < w ? xx : w - 1)];
      }
    }
#pragma unroll
    for (int r = 0; r < DT_ROWS; ++r) {
#pragma unroll
      for (int c = 0; c < DT_TW / DT_LANES; ++c) {
        const int yy = y0 + r, xx = x0 + c * DT_LANES + lane;
        tile[r][c * DT_LANES + lane] = (yy < h && xx < w) ? (unsigned int)v[r][c] : DT_NONE;
      }
    }
    __syncthreads();
    if (live) {
      const int jn = w - x0 < DT_TW ? w - x0 : DT_TW;
      for (int j = 0; j < jn; ++j) {
        const unsigned int gu = tile[lane][j];
        if (gu == DT_NONE) continue;         // no site in this column: it is no parabola
        const int u = x0 + j;
        while (q >= 0 && dt_f(tt, ts, tg) > dt_f(tt, u, gu)) pop();
        if (q < 0) {
          push(u, 0, gu);
        } else {
          // the last column at which the top is still no higher than u: floor((u^2 + gu^2 - (s^2 + gs^2)) / (2 (u - s))).  u, s and
          // both g are below 2^15 (h, w <= 32768), so either bracket is below 2^31; the loop above left f(t, s) <= f(t, u) at
          // t >= 0, so the difference is >= 2 t (u - s) >= 0: unsigned 32-bit arithmetic is exact here (64-bit terms give the same
          // values and measured 3 % slower on a 6000 x 6000 map).
          const unsigned int num = dt_f(u, 0, gu) - dt_f(ts, 0, tg);
          const unsigned int sep = num / (unsigned int)(2 * (u - ts));
          if (sep + 1u < (unsigned int)w) push(u, (int)sep + 1, gu);
        }
      }
    }
    __syncthreads();
  }
  for (int x0 = ((w - 1) / DT_TW) * DT_TW; x0 >= 0; x0 -= DT_TW) {
    if (live) {
      const int jl = w - 1 - x0 < DT_TW - 1 ? w - 1 - x0 : DT_TW - 1;
      for (int j = jl; j >= 0; --j) {
        const int xx = x0 + j;
        tile[lane][j] = q < 0 ? (unsigned int)DRS_DT_INF : dt_f(xx, ts, tg);
        if (q >= 0 && xx == tt) pop();
      }
    }
    __syncthreads();
    for (int r = 0; r < DT_ROWS; ++r) {
      for (int c = 0; c < DT_TW; c += DT_LANES) {
        const int yy = y0 + r, xx = x0 + c + lane;
        if (yy < h && xx < w) out[(size_t)yy * w + xx] = tile[r][c + lane];
      }
    }
    __syncthreads();
  }
}

inline size_t dt_align(size_t v) { return (v + 15) & ~(size_t)15; }

struct DtLayout {
  size_t g, first, last, stack, total;
};

DtLayout dt_layout(int h, int w, int batch, size_t off) {
  const size_t n = (size_t)h * w, ns = (size_t)((h + DT_STRIP - 1) / DT_STRIP);
  DtLayout l;
  l.g = off;
  off += dt_align(batch * n * 2);
  l.first = off;
  off += dt_align(batch * ns * w * 4);
  l.last = off;
  off += dt_align(batch * ns * w * 4);
  l.stack = off;
  off += dt_align(batch * n * 8);
  l.total = off;
  return l;
}

bool dt_shape_ok(int h, int w) {
  return h >= 1 && w >= 1 && h <= DT_MAX_SIDE && w <= DT_MAX_SIDE && (long long)h * w <= DT_MAX_PIX;
}

// the scratch as the caller gave it, from its first 16-byte boundary on (the queries count the slack)
char* dt_base(void* scratch) { return (char*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15); }

void dt_bind(DtArgs& a, int h, int w, char* base, const DtLayout& l) {
  a.h = h;
  a.w = w;
  a.nstrips = (h + DT_STRIP - 1) / DT_STRIP;
  a.g = (unsigned short*)(base + l.g);
  a.first = (int*)(base + l.first);
  a.last = (int*)(base + l.last);
  a.stack = (unsigned long long*)(base + l.stack);
}

int dt_launch(const DtArgs& a, int batch, hipStream_t stream) {
  const dim3 cols((a.w + DT_COLS - 1) / DT_COLS, a.nstrips, batch);
  DRS_LAUNCH(dt_strip_ends_kernel, cols, dim3(DT_COLS), 0, stream, a);
  int rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(dt_columns_kernel, cols, dim3(DT_COLS), 0, stream, a);
  rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(dt_rows_kernel, dim3((a.h + DT_ROWS - 1) / DT_ROWS, batch), dim3(DT_LANES), 0, stream, a);
  return DRS_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------- the surface table
struct SfArgs {
  const unsigned char* truth;
  const unsigned char* pred;
  int h, w, K, ignore_label, cls;
  unsigned int n;
  unsigned char* edge[2];                   // [h][w] each: truth, veiled prediction
  unsigned int* cnt;                        // [2][8]: contour pixels per class and map
  const unsigned int* d2[2];                // distances to the class's contour in truth, in the veiled prediction
  unsigned long long* table;
};

__device__ __forceinline__ int sf_pred_byte(const SfArgs& a, size_t i) {
  return (a.ignore_label >= 0 && a.truth[i] == a.ignore_label) ? a.ignore_label : a.pred[i];
}

// edge[m][p] = some 4-neighbour of p inside the map carries another byte in map m; cnt[m][c] = the contour pixels of class c
__global__ void __launch_bounds__(SF_THREADS) sf_edges_kernel(const SfArgs a) {
  __shared__ unsigned int cnt[2 * SF_MAX_K];
  if (threadIdx.x < 2 * SF_MAX_K) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned int w = (unsigned int)a.w, h = (unsigned int)a.h;
  for (unsigned int i = blockIdx.x * SF_THREADS + threadIdx.x; i < a.n; i += gridDim.x * SF_THREADS) {
    const unsigned int y = i / w, x = i - y * w;
    const int bt = a.truth[i], bp = sf_pred_byte(a, i);
    bool et = false, ep = false;
    if (y > 0) { et |= a.truth[i - w] != bt; ep |= sf_pred_byte(a, i - w) != bp; }
    if (y + 1 < h) { et |= a.truth[i + w] != bt; ep |= sf_pred_byte(a, i + w) != bp; }
    if (x > 0) { et |= a.truth[i - 1] != bt; ep |= sf_pred_byte(a, i - 1) != bp; }
    if (x + 1 < w) { et |= a.truth[i + 1] != bt; ep |= sf_pred_byte(a, i + 1) != bp; }
    a.edge[0][i] = et ? 1 : 0;
    a.edge[1][i] = ep ? 1 : 0;
    if (et && bt < a.K && bt != a.ignore_label) atomicAdd(&cnt[bt], 1u);
    if (ep && bp < a.K && bp != a.ignore_label) atomicAdd(&cnt[SF_MAX_K + bp], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 2 * SF_MAX_K && cnt[threadIdx.x]) atomicAdd(&a.cnt[threadIdx.x], cnt[threadIdx.x]);
}

// b = the smallest integer with 16 D <= b^2; f = floor(sqrt(D 2^20)).  A double square root, then the integer fix-up.
__device__ __forceinline__ void sf_bin(unsigned int D, unsigned int& b, unsigned long long& f) {
  const unsigned long long v = 16ULL * D, s = (unsigned long long)D << 20;
  unsigned long long r = (unsigned long long)sqrt((double)v);
  while (r * r < v) ++r;
  while (r > 0 && (r - 1) * (r - 1) >= v) --r;
  b = (unsigned int)r;
  f = (unsigned long long)sqrt((double)s);
  while (f * f > s) --f;
  while ((f + 1) * (f + 1) <= s) ++f;
}

// the two directions of class a.cls, both contour sets non-empty: 32-bit LDS counters per workgroup, the non-zero ones flushed with
// 64-bit atomics, as boundary_histogram_kernel does
__global__ void __launch_bounds__(SF_THREADS) sf_gather_kernel(const SfArgs a) {
  if (a.cnt[a.cls] == 0u || a.cnt[SF_MAX_K + a.cls] == 0u) return;
  __shared__ unsigned int tab[2 * SF_BINS];
  __shared__ unsigned long long fsum[2];
  for (int j = threadIdx.x; j < 2 * SF_BINS; j += SF_THREADS) tab[j] = 0u;
  if (threadIdx.x < 2) fsum[threadIdx.x] = 0ULL;
  __syncthreads();
  unsigned long long f[2] = {0ULL, 0ULL};
  for (unsigned int i = blockIdx.x * SF_THREADS + threadIdx.x; i < a.n; i += gridDim.x * SF_THREADS) {
    const bool walk0 = a.edge[0][i] && a.truth[i] == a.cls, walk1 = a.edge[1][i] && sf_pred_byte(a, i) == a.cls;
    if (walk0) {
      unsigned int b;
      unsigned long long fv;
      sf_bin(a.d2[1][i], b, fv);
      atomicAdd(&tab[b < SF_BINS - 1 ? b : SF_BINS - 1], 1u);
      f[0] += fv;
    }
    if (walk1) {
      unsigned int b;
      unsigned long long fv;
      sf_bin(a.d2[0][i], b, fv);
      atomicAdd(&tab[SF_BINS + (b < SF_BINS - 1 ? b : SF_BINS - 1)], 1u);
      f[1] += fv;
    }
  }
  if (f[0]) atomicAdd(&fsum[0], f[0]);
  if (f[1]) atomicAdd(&fsum[1], f[1]);
  __syncthreads();
  const size_t row = SF_BINS + 2;
  for (int j = threadIdx.x; j < 2 * SF_BINS; j += SF_THREADS) {
    const unsigned int v = tab[j];
    const int dir = j / SF_BINS, bin = j - dir * SF_BINS;
    if (v) atomicAdd(&a.table[((size_t)dir * a.K + a.cls) * row + bin], (unsigned long long)v);
  }
  if (threadIdx.x < 2 && fsum[threadIdx.x]) atomicAdd(&a.table[((size_t)threadIdx.x * a.K + a.cls) * row + SF_BINS], fsum[threadIdx.x]);
}

// the walked pixels of a class whose counterpart set is empty
__global__ void __launch_bounds__(64) sf_unsited_kernel(const SfArgs a) {
  const int c = threadIdx.x;
  if (c >= a.K || c == a.ignore_label) return;
  const unsigned int ct = a.cnt[c], cp = a.cnt[SF_MAX_K + c];
  const size_t row = SF_BINS + 2;
  if (ct && !cp) atomicAdd(&a.table[((size_t)0 * a.K + c) * row + SF_BINS + 1], (unsigned long long)ct);
  if (cp && !ct) atomicAdd(&a.table[((size_t)1 * a.K + c) * row + SF_BINS + 1], (unsigned long long)cp);
}

struct SfLayout {
  size_t cnt, edge[2], d2[2];
  DtLayout dt;
};

SfLayout sf_layout(int h, int w) {
  const size_t n = (size_t)h * w;
  SfLayout l;
  size_t off = 0;
  l.cnt = off;
  off += 256;
  for (int m = 0; m < 2; ++m) { l.edge[m] = off; off += dt_align(n); }
  for (int m = 0; m < 2; ++m) { l.d2[m] = off; off += dt_align(n * 4); }
  l.dt = dt_layout(h, w, DT_BATCH, off);
  return l;
}

}  // namespace

extern "C" {

size_t drs_distance_scratch_bytes(int h, int w) {
  if (!dt_shape_ok(h, w)) return 0;
  return dt_layout(h, w, 1, 0).total + 16;
}

int drs_distance_transform(const unsigned char* map, const unsigned char* veil, int veil_label, int h, int w, int mode, int cls,
                           unsigned int* d2, void* scratch, size_t scratch_bytes, void* stream) {
  if (!map || !d2 || !scratch || !dt_shape_ok(h, w) || mode < DRS_DT_CLASS || mode > DRS_DT_CONTOUR || cls < 0 || cls > 255) return DRS_ERR_ARG;
  if (veil && (veil_label < 0 || veil_label > 255)) return DRS_ERR_ARG;
  if (scratch_bytes < drs_distance_scratch_bytes(h, w)) return DRS_ERR_ARG;
  DtArgs a = {};
  dt_bind(a, h, w, dt_base(scratch), dt_layout(h, w, 1, 0));
  a.src[0].map = map;
  a.src[0].veil = veil;
  a.src[0].veil_label = veil ? veil_label : -1;
  a.src[0].mode = mode;
  a.src[0].cls = cls;
  a.d2[0] = d2;
  return dt_launch(a, 1, (hipStream_t)stream);
}

size_t drs_surface_scratch_bytes(int h, int w) {
  if (!dt_shape_ok(h, w)) return 0;
  return sf_layout(h, w).dt.total + 16;
}

int drs_surface_histogram(const unsigned char* truth, const unsigned char* pred, int h, int w, int K, int ignore_label,
                          unsigned long long* table, void* scratch, size_t scratch_bytes, void* stream) {
  if (!truth || !pred || !table || !scratch || !dt_shape_ok(h, w) || K < 2 || K > SF_MAX_K || ignore_label < -1 || ignore_label > 255)
    return DRS_ERR_ARG;
  if (scratch_bytes < drs_surface_scratch_bytes(h, w)) return DRS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const SfLayout l = sf_layout(h, w);
  char* base = dt_base(scratch);
  SfArgs s = {};
  s.truth = truth;
  s.pred = pred;
  s.h = h;
  s.w = w;
  s.K = K;
  s.ignore_label = ignore_label;
  s.n = (unsigned int)((size_t)h * w);
  s.cnt = (unsigned int*)(base + l.cnt);
  for (int m = 0; m < 2; ++m) {
    s.edge[m] = (unsigned char*)(base + l.edge[m]);
    s.d2[m] = (const unsigned int*)(base + l.d2[m]);
  }
  s.table = table;
  const unsigned int blocks = (s.n + SF_THREADS - 1) / SF_THREADS;
  const dim3 grid(blocks < (unsigned int)SF_MAX_GRID ? blocks : (unsigned int)SF_MAX_GRID);
  (void)hipGetLastError();
  if (hipMemsetAsync(s.cnt, 0, 2 * SF_MAX_K * sizeof(unsigned int), st) != hipSuccess) return DRS_ERR_HIP;
  DRS_LAUNCH(sf_edges_kernel, grid, dim3(SF_THREADS), 0, st, s);
  int rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DtArgs a = {};
  dt_bind(a, h, w, base, l.dt);
  a.cnt = s.cnt;
  for (int m = 0; m < 2; ++m) {
    a.src[m].map = m ? pred : truth;
    a.src[m].veil = (m && ignore_label >= 0) ? truth : nullptr;
    a.src[m].veil_label = (m && ignore_label >= 0) ? ignore_label : -1;
    a.src[m].edge = s.edge[m];
    a.src[m].mode = DRS_DT_CONTOUR;
    a.d2[m] = (unsigned int*)(base + l.d2[m]);
  }
  for (int c = 0; c < K; ++c) {
    if (c == ignore_label) continue;
    a.cnt_cls = c;
    a.src[0].cls = a.src[1].cls = c;
    rc = dt_launch(a, DT_BATCH, st);
    if (rc != DRS_OK) return rc;
    s.cls = c;
    DRS_LAUNCH(sf_gather_kernel, grid, dim3(SF_THREADS), 0, st, s);
    rc = DRS_LAUNCH_CHECK();
    if (rc != DRS_OK) return rc;
  }
  DRS_LAUNCH(sf_unsited_kernel, dim3(1), dim3(64), 0, st, s);
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
