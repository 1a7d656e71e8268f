// Boundary-quality counts of a (truth, prediction) pair of label maps (opt-in; include/drs.h: drs_boundary_distance,
// drs_boundary_histogram): the squared distance of every pixel to the nearest pixel of its own map that carries another
// byte, inside a (2R+1)^2 window and inside the map, binned against d_i^2 in both maps and counted per (truth bin, prediction bin,
// truth label, prediction label).  Trimap accuracy (Kohli et al. 2009) and Boundary IoU (Cheng et al. 2021) are sums over that table
// (metrics.boundary_scores).  tests/boundary_ref.py states the rule in numpy.  Everything is integer: nothing is rounded anywhere.
// Also here, at the end: the boundary weight map of a training step's label patches (drs_patch_boundary_weight), which
// shares the tile geometry and the distance convention but not the scan.
#include "drs_common.hpp"
#include "../../include/drs.h"
#include <cmath>

namespace {

constexpr int BD_MAX_K = 8, BD_MAX_N = 8, BD_MAX_R = 16;
constexpr int BD_TX = 64;                   // output columns of a tile: one wave per row, its lanes on consecutive LDS cells
constexpr int BD_TY = 32;                   // output rows of a tile
constexpr int BD_THREADS = 256;
constexpr int BD_PIX = BD_TX * BD_TY / BD_THREADS;      // 8 pixels per thread: rows q * 8 .. q * 8 + 7 of column lx
constexpr int BD_LW = BD_TX + 2 * BD_MAX_R, BD_LH = BD_TY + 2 * BD_MAX_R;
constexpr int BD_NONE = 255;                // "no other byte within R columns of this row"; a real run distance is 1..16
constexpr int BD_INF = 1 << 30;             // D^2 of a pixel whose window holds no other byte
constexpr int BD_MAX_GRID = 2048;           // persistent workgroups: each walks tiles blockIdx.x, + gridDim.x, ...
constexpr int BD_TAB = (BD_MAX_N + 1) * (BD_MAX_N + 1) * BD_MAX_K * BD_MAX_K;      // 5184 counters = 20.25 KiB

// One map's tile in LDS.  lab: the bytes of the tile plus a halo of R ([TY + 2R][TX + 2R], row stride TX + 2R); a position outside
// the map holds a 0 that nothing reads as a label: the scans below clamp their bounds to the map instead, since any byte is a legal
// label and none can serve as a sentinel.  cell: for the tile's own columns of every staged row ([TY + 2R][TX]), the byte and, in the
// high half, the distance along the ROW to the nearest column inside the map, at most R away, that holds another byte (BD_NONE if
// there is none).
struct BdTile {
  unsigned char lab[BD_LH * BD_LW];
  unsigned short cell[BD_LH * BD_TX];
};

__device__ __forceinline__ void bd_stage_labels(const unsigned char* __restrict__ map, int h, int w, int y0, int x0, int R, BdTile& s) {
  const int LW = BD_TX + 2 * R, LH = BD_TY + 2 * R;
  const float rcp = 1.0f / (float)LW;
  for (int idx = threadIdx.x; idx < LW * LH; idx += BD_THREADS) {
    int ry, rx;
    divmod24(idx, LW, rcp, ry, rx);
    const int gy = y0 - R + ry, gx = x0 - R + rx;
    const bool inside = gy >= 0 && gy < h && gx >= 0 && gx < w;
    s.lab[idx] = inside ? map[(size_t)gy * w + gx] : (unsigned char)0;
  }
}

// (after a barrier behind bd_stage_labels) the row pass: the window scan is separable because the byte a pixel p is compared with is
// its own.  In row r of p's window let l be the byte straight above / below p (column x).  If l != m[p] the row's nearest other byte
// is at dx = 0.  If l == m[p], "another byte than m[p]" and "another byte than l" are the same set, and its nearest member is the row
// distance of the cell (r, x) -- which does not depend on p.  So every cell's row distance is found once (at most 2R byte reads, leaving
// at the first hit), and a pixel then reads 2R + 1 cells of its column instead of (2R + 1)^2 bytes: the same minimum, exactly.
__device__ __forceinline__ void bd_stage_cells(int w, int y0, int x0, int R, BdTile& s) {
  const int LW = BD_TX + 2 * R, LH = BD_TY + 2 * R;
  for (int idx = threadIdx.x; idx < LH * BD_TX; idx += BD_THREADS) {
    const int ry = idx / BD_TX, c = idx - ry * BD_TX;
    const int gx = x0 + c;
    const unsigned char* row = s.lab + ry * LW + c + R;
    const int l = row[0];
    const int la = gx < R ? gx : R, ra = w - 1 - gx < R ? w - 1 - gx : R;          // the columns of the map on either side (ra < 0 past it)
    int hd = BD_NONE;
    for (int a = 1; a <= R; ++a) {
      if ((a <= la && row[-a] != l) || (a <= ra && row[a] != l)) { hd = a; break; }
    }
    s.cell[idx] = (unsigned short)(l | (hd << 8));
  }
}

// D^2 of the pixel at tile position (ly, lx), image row gy = y0 + ly < h: the one statement of the distance rule, used by both maps of
// the histogram kernel and by the distance kernel.  The rows outside the map are never read.
__device__ __forceinline__ int bd_d2(const BdTile& s, int h, int gy, int ly, int lx, int R) {
  const unsigned short* col = s.cell + (ly + R) * BD_TX + lx;
  const int mine = col[0] & 255;
  const int lo = gy < R ? -gy : -R, hi = h - 1 - gy < R ? h - 1 - gy : R;
  int best = BD_INF;
  for (int dy = lo; dy <= hi; ++dy) {
    const int c = col[dy * BD_TX];
    const int d = (c & 255) != mine ? 0 : (c >> 8);
    const int cand = dy * dy + d * d;
    if (d <= R && cand < best) best = cand;
  }
  return best;
}

struct BdArgs {
  const unsigned char* truth;
  const unsigned char* pred;                // null in the distance kernel
  int h, w, K, ignore_label, n, R;
  int dsq[BD_MAX_N];                        // d_i^2, ascending
  int tiles_x;
  unsigned long long ntiles;
  unsigned long long* hist;
  unsigned short* d2;
};

__device__ __forceinline__ int bd_bin(const BdArgs& a, int d2) {
  int b = a.n;
#pragma unroll
  for (int i = BD_MAX_N - 1; i >= 0; --i)
    if (i < a.n && d2 <= a.dsq[i]) b = i;
  return b;
}

// hist[bin_truth][bin_pred][truth][pred] += 1 per counted pixel.  A workgroup walks its tiles and counts into a table of 32-bit LDS
// counters, flushed once at its end with 64-bit atomics (only the non-zero entries), as the other histogram kernels do.  Most pixels
// of a real map land in the one cell [n][n][c][c]: a thread therefore keeps the cell of its last pixel and a run length in registers,
// across its 8 pixels of a tile and across tiles, and touches LDS only when the cell changes -- an interior thread adds once per launch.
// The 32-bit counters hold: a workgroup sees at most ceil(ntiles / grid) * 2048 < 2^32 pixels (ntiles < 2^31 for h w < 2^40).
__global__ void __launch_bounds__(BD_THREADS) boundary_histogram_kernel(const BdArgs a) {
  __shared__ BdTile tile[2];
  __shared__ unsigned int tab[BD_TAB];
  const int nb = a.n + 1, K = a.K;
  const int cells = nb * nb * K * K;
  for (int j = threadIdx.x; j < cells; j += BD_THREADS) tab[j] = 0u;
  __syncthreads();
  const int lx = threadIdx.x & (BD_TX - 1), q = threadIdx.x / BD_TX;
  int run_cell = -1;
  unsigned run = 0u;
  for (unsigned long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int tyi = (int)(t / (unsigned long long)a.tiles_x);
    const int y0 = tyi * BD_TY, x0 = (int)(t - (unsigned long long)tyi * a.tiles_x) * BD_TX;
    bd_stage_labels(a.truth, a.h, a.w, y0, x0, a.R, tile[0]);
    bd_stage_labels(a.pred, a.h, a.w, y0, x0, a.R, tile[1]);
    __syncthreads();
    bd_stage_cells(a.w, y0, x0, a.R, tile[0]);
    bd_stage_cells(a.w, y0, x0, a.R, tile[1]);
    __syncthreads();
    // (the next tile's label pass writes `lab` only, and its cell pass waits behind a barrier every thread reaches after this loop)
    const int gx = x0 + lx;
    if (gx < a.w) {
      for (int i = 0; i < BD_PIX; ++i) {
        const int ly = q * BD_PIX + i, gy = y0 + ly;
        if (gy >= a.h) break;
        const int ci = (ly + a.R) * BD_TX + lx;
        const int yt = tile[0].cell[ci] & 255, yp = tile[1].cell[ci] & 255;
        if (yt == a.ignore_label || yt >= K || yp >= K) continue;            // exactly the pixels drs_confusion counts
        const int bt = bd_bin(a, bd_d2(tile[0], a.h, gy, ly, lx, a.R));
        const int bp = bd_bin(a, bd_d2(tile[1], a.h, gy, ly, lx, a.R));
        const int cell = ((bt * nb + bp) * K + yt) * K + yp;
        if (cell == run_cell) {
          ++run;
        } else {
          if (run) atomicAdd(&tab[run_cell], run);
          run_cell = cell;
          run = 1u;
        }
      }
    }
  }
  if (run) atomicAdd(&tab[run_cell], run);
  __syncthreads();
  for (int j = threadIdx.x; j < cells; j += BD_THREADS) {
    const unsigned v = tab[j];
    if (v) atomicAdd(&a.hist[j], (unsigned long long)v);
  }
}

// d2[y][x] = min(D^2, 65535) of one map (a.truth), through the same staging and the same bd_d2
__global__ void __launch_bounds__(BD_THREADS) boundary_distance_kernel(const BdArgs a) {
  __shared__ BdTile tile;
  const int lx = threadIdx.x & (BD_TX - 1), q = threadIdx.x / BD_TX;
  for (unsigned long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int tyi = (int)(t / (unsigned long long)a.tiles_x);
    const int y0 = tyi * BD_TY, x0 = (int)(t - (unsigned long long)tyi * a.tiles_x) * BD_TX;
    bd_stage_labels(a.truth, a.h, a.w, y0, x0, a.R, tile);
    __syncthreads();
    bd_stage_cells(a.w, y0, x0, a.R, tile);
    __syncthreads();
    const int gx = x0 + lx;
    if (gx < a.w) {
      for (int i = 0; i < BD_PIX; ++i) {
        const int ly = q * BD_PIX + i, gy = y0 + ly;
        if (gy >= a.h) break;
        const int v = bd_d2(tile, a.h, gy, ly, lx, a.R);
        a.d2[(size_t)gy * a.w + gx] = (unsigned short)(v < 65535 ? v : 65535);
      }
    }
  }
}

// tiles and grid of an h x w map; false where h w >= 2^40 (what the 32-bit LDS counters and the tile index are sized for)
bool bd_geometry(int h, int w, BdArgs& a, unsigned& grid) {
  if (h < 1 || w < 1 || (unsigned long long)h * (unsigned long long)w >= (1ULL << 40)) return false;
  a.h = h;
  a.w = w;
  a.tiles_x = (w + BD_TX - 1) / BD_TX;          // (h, w < 2^31: no overflow; the product of the two tile counts stays below 2^31)
  a.ntiles = (unsigned long long)a.tiles_x * (unsigned long long)((h + BD_TY - 1) / BD_TY);
  grid = a.ntiles < (unsigned long long)BD_MAX_GRID ? (unsigned)a.ntiles : (unsigned)BD_MAX_GRID;
  return true;
}

// ---------------------------------------------------------------------------- boundary weight map of a step's label patches
// (opt-in; include/drs.h: drs_patch_boundary_weight; tests/boundary_weight_ref.py states the rule in numpy.)
// lab, valid: [B][S][S] bytes, valid may be null ("all valid").  For a valid pixel p, D2(p) = min dy^2 + dx^2 over the positions
// q = p + (dy, dx) with |dy|, |dx| <= R, q inside the SAME patch, q valid and lab[q] != lab[p]; infinite when there is none or when p
// is invalid.  weight = 1 where D2 is infinite, else (float)(1 + a exp(-D2 c)) evaluated in fp64 and rounded once.  The patch edge is
// no boundary, a byte is just a byte, and an invalid q never counts as "different" (rotated-in fill draws no contour).
// The row / column scan of bd_d2 does not carry over: when the cell straight above p is invalid it is not "different", and it has
// no byte whose row distance would say anything about the bytes that differ from p's.  So the window is scanned directly, in LDS, ring by
// ring: ring r (Chebyshev distance r) holds squared distances r^2 .. 2 r^2 only, so the scan leaves at the first ring with
// r^2 >= the minimum so far -- an interior pixel next to a contour reads a ring or two, and only pixels far from any contour read the
// whole (2R + 1)^2 window.
// One staged cell: the byte, or BW_OUT for a position outside the patch or an invalid one -- a 16-bit value no byte equals, so
// "inside, valid, another byte" is two compares and no bound is clamped.
constexpr unsigned short BW_OUT = 0xFFFFu;

struct BwArgs {
  const unsigned char* lab;
  const unsigned char* valid;
  int B, S, R, tiles_x, tiles_per_patch, ntiles;
  double a, c;
  unsigned short* d2;
  float* weight;
};

__global__ void __launch_bounds__(BD_THREADS) patch_boundary_weight_kernel(const BwArgs a) {
  __shared__ unsigned short cell[BD_LH * BD_LW];
  const int R = a.R, S = a.S;
  const int LW = BD_TX + 2 * R, LH = BD_TY + 2 * R;
  const float rcp = 1.0f / (float)LW;
  const int lx = threadIdx.x & (BD_TX - 1), q = threadIdx.x / BD_TX;
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int b = t / a.tiles_per_patch, rem = t - b * a.tiles_per_patch;
    const int tyi = rem / a.tiles_x;
    const int y0 = tyi * BD_TY, x0 = (rem - tyi * a.tiles_x) * BD_TX;
    const int base = b * S * S;              // (B S S < 2^24: every index fits an int)
    for (int idx = threadIdx.x; idx < LW * LH; idx += BD_THREADS) {
      int ry, rx;
      divmod24(idx, LW, rcp, ry, rx);
      const int gy = y0 - R + ry, gx = x0 - R + rx;
      unsigned short v = BW_OUT;
      if (gy >= 0 && gy < S && gx >= 0 && gx < S) {
        const int g = base + gy * S + gx;
        if (!a.valid || a.valid[g]) v = a.lab[g];
      }
      cell[idx] = v;
    }
    __syncthreads();
    const int gx = x0 + lx;
    if (gx < S) {
      for (int i = 0; i < BD_PIX; ++i) {
        const int ly = q * BD_PIX + i, gy = y0 + ly;
        if (gy >= S) break;
        const unsigned short* ctr = cell + (ly + R) * LW + lx + R;
        const unsigned short mine = ctr[0];
        int best = BD_INF;
        if (mine != BW_OUT) {
          auto look = [&](int dy, int dx) {
            const unsigned short v = ctr[dy * LW + dx];
            const int cand = dy * dy + dx * dx;
            if (v != mine && v != BW_OUT && cand < best) best = cand;
          };
          for (int r = 1; r <= R && best > r * r; ++r) {
            for (int s = -r; s <= r; ++s) {
              look(-r, s);
              look(r, s);
            }
            for (int s = 1 - r; s < r; ++s) {
              look(s, -r);
              look(s, r);
            }
          }
        }
        const int g = base + gy * S + gx;
        if (a.d2) a.d2[g] = (unsigned short)(best < 65535 ? best : 65535);
        a.weight[g] = best == BD_INF ? 1.0f : (float)(1.0 + a.a * exp(-(double)best * a.c));
      }
    }
    __syncthreads();              // the next tile's staging overwrites the cells this one still reads
  }
}

}  // namespace

extern "C" {

int drs_boundary_distance(const unsigned char* map, int h, int w, int R, unsigned short* d2, void* stream) {
  BdArgs a = {};
  unsigned grid;
  if (!map || !d2 || R < 1 || R > BD_MAX_R || !bd_geometry(h, w, a, grid)) return DRS_ERR_ARG;
  a.truth = map;
  a.d2 = d2;
  a.R = R;
  DRS_LAUNCH(boundary_distance_kernel, dim3(grid), dim3(BD_THREADS), 0, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

int drs_boundary_histogram(const unsigned char* truth, const unsigned char* pred, int h, int w, int K, int ignore_label,
                           const int* distances, int n, unsigned long long* hist, void* stream) {
  BdArgs a = {};
  unsigned grid;
  if (!truth || !pred || !distances || !hist || K < 2 || K > BD_MAX_K || n < 1 || n > BD_MAX_N || !bd_geometry(h, w, a, grid))
    return DRS_ERR_ARG;
  for (int i = 0; i < n; ++i) {
    const int d = distances[i];
    if (d < 1 || d > BD_MAX_R || (i && d <= distances[i - 1])) return DRS_ERR_ARG;
    a.dsq[i] = d * d;
  }
  a.truth = truth;
  a.pred = pred;
  a.K = K;
  a.ignore_label = ignore_label;
  a.n = n;
  a.R = distances[n - 1];
  a.hist = hist;
  DRS_LAUNCH(boundary_histogram_kernel, dim3(grid), dim3(BD_THREADS), 0, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

int drs_patch_boundary_weight(const unsigned char* lab, const unsigned char* valid, int B, int S, int R, double a, double c,
                              unsigned short* d2_out, float* weight_out, void* stream) {
  if (!lab || !weight_out || B < 1 || S < 1 || S >= (1 << 12) || (long long)B * S * S >= (1LL << 24) || R < 1 || R > BD_MAX_R) return DRS_ERR_ARG;
  if (!std::isfinite(a) || a < -1.0 || a > 64.0 || !std::isfinite(c) || !(c > 0.0)) return DRS_ERR_ARG;
  BwArgs k = {};
  k.lab = lab; k.valid = valid; k.B = B; k.S = S; k.R = R; k.a = a; k.c = c; k.d2 = d2_out; k.weight = weight_out;
  k.tiles_x = (S + BD_TX - 1) / BD_TX;
  k.tiles_per_patch = k.tiles_x * ((S + BD_TY - 1) / BD_TY);
  k.ntiles = B * k.tiles_per_patch;              // (< 2^24: a tile holds at least one pixel)
  DRS_LAUNCH(patch_boundary_weight_kernel, dim3(k.ntiles < BD_MAX_GRID ? k.ntiles : BD_MAX_GRID), dim3(BD_THREADS), 0,
             (hipStream_t)stream, k);
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
