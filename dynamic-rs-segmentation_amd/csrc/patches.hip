// Patch materialisation and whole-tile stitching on gfx950 (HBM-bound gather / scatter-free accumulate).
//
// Reference call sites (/root/reference/isprs_dilated_random.py):
//   dynamically_create_patches :245-334  (crop, border shift-back done by the host, rotate / noise / flip augmentation)
//   normalize_images           :74-81    ((x - mean[c]) / std[c] for c = 0,1,2 ONLY)
//   create_patches_per_map     :337-400  (same gather, window positions from the host)
//   overlap-add of logits      :1261-1284 / :1925-1949, arg-max of the average
//   (and, beside the reference's windows, the opt-in overlap-tile inference: exact cores of whole-net tiles, drs_tile_place;
//    its dihedral test-time augmentation: drs_crop_dihedral, drs_tile_place_dihedral; its multi-scale test-time augmentation:
//    drs_crop_resampled, drs_resample_accumulate; and, for training, the crop with scale jitter: drs_crop_normalize_scaled)
//
// The crop writes straight into the zero-haloed, channel-padded input slab of conv1, so no separate pad/normalise
// pass exists.  Arithmetic on pixel values is fp64 (the reference normalises float64 patches, then feeds float32),
// rounded once to fp32 on the store, so the result is bit-identical to the reference's feed.
#include "drs_common.hpp"
#include <cfloat>

// Everything in this file restates host arithmetic that the reference does in numpy / scipy and is held to it BIT FOR BIT: no
// multiply-add may be fused.  hipcc contracts a * b + c into an fma by default, and HIP's __dmul_rn / __dadd_rn are no
// barrier against that (they are folded into fmas all the same): the rotation's source coordinate ((i m00) + j m01) + off came out as fma(j, m01, i m00) + off, which
// picks the other neighbour than scipy.ndimage at exact ties (multiples of 15 / 45 degrees at some sides: tests/fuzz/check_rotation.py).
#pragma clang fp contract(off)

namespace {

struct CropArgs {
  const void* tiles;            // pool of HWC tiles (double or float)
  const unsigned char* labels;  // pool of HW label maps
  const long long* tile_off;    // [nmaps] element offset of each tile in the pool
  const long long* lab_off;     // [nmaps]
  const int* tile_h; const int* tile_w;
  int C;                        // real channels
  const int* inst;              // [B][4]: map, x (row), y (col), flip (0 none, 1 flipud, 2 fliplr)
  const double* rot;            // [B][6]: m00 m01 m10 m11 off0 off1 (scipy affine, output->input) or null
  const unsigned char* rot_on;  // [B] or null
  const double* noise;          // [B][S][S][C] additive noise (pre-flip coordinates) or null
  const unsigned char* noise_on;  // [B] or null
  unsigned long long seed;      // device noise (Philox) when noise == null and noise_on[b]
  int quantize_f16;             // coffee:293 + :67-74: value, (value - mean) and (... / std) each rounded to float16
  int b0;                       // index of this call's first patch in the global batch: the noise of a patch does not depend on how the batch is sharded
  int void_label;               // pixels carrying this label are masked out too (contest:235-239); -1 = none
  double mean[3], stdv[3];
  float* out; int S, P, ld;     // conv1 input slab [B][S+2P][S+2P][ld]
  unsigned char* out_lab;       // [B][S][S]
  unsigned char* out_mask;      // [B][S][S] validity (0 where the rotation pulled in fill)
};

// Philox-4x32-10 -> two N(0,1) (Box-Muller) per call, keyed by (seed, element index)
__device__ __forceinline__ void philox(unsigned long long seed, unsigned long long ctr, unsigned (&o)[4]) {
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  unsigned c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32), c2 = 0x1234567u, c3 = 0x89abcdefu;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ double normal_from(unsigned a, unsigned b) {
  const double u1 = ((double)a + 1.0) * (1.0 / 4294967296.0), u2 = (double)b * (1.0 / 4294967296.0);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

template <typename T>
__global__ void crop_kernel(const CropArgs a) {
  const int Sp = a.S + 2 * a.P;
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= Sp) return;
  const int b = blockIdx.y / Sp, yy = blockIdx.y - b * Sp;
  float* dst = a.out + ((size_t)(b * Sp + yy) * Sp + xx) * a.ld;
  const int i = yy - a.P, j = xx - a.P;
  const bool inside = i >= 0 && i < a.S && j >= 0 && j < a.S;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (inside) {
    const int map = a.inst[4 * b], px = a.inst[4 * b + 1], py = a.inst[4 * b + 2], flip = a.inst[4 * b + 3];
    // undo the flip (applied last by the reference), then the rotation (applied first)
    const int fi = flip == 1 ? a.S - 1 - i : i, fj = flip == 2 ? a.S - 1 - j : j;
    int si = fi, sj = fj;
    bool valid = true;
    if (a.rot_on && a.rot_on[b]) {
      const double* m = a.rot + 6 * b;
      // scipy.ndimage geometric transform, order 0: in = M . out + offset (no FMA contraction), nearest = floor(c + 0.5)
      // (plain operators under this file's `fp contract(off)`: every product and every sum rounded on its own, as in ndimage's C)
      const double p00 = (double)fi * m[0], p01 = (double)fj * m[1], p10 = (double)fi * m[2], p11 = (double)fj * m[3];
      double c0 = 0.0 + p00;
      c0 = c0 + p01;
      c0 = c0 + m[4];
      double c1 = 0.0 + p10;
      c1 = c1 + p11;
      c1 = c1 + m[5];
      valid = !(c0 < 0.0 || c0 > (double)(a.S - 1) || c1 < 0.0 || c1 > (double)(a.S - 1));
      si = (int)floor(c0 + 0.5);
      sj = (int)floor(c1 + 0.5);
    }
    const size_t opix = ((size_t)b * a.S + i) * a.S + j;
    unsigned char lab = 0;
    const T* src = nullptr;
    if (valid) {
      const int W = a.tile_w[map];
      src = reinterpret_cast<const T*>(a.tiles) + a.tile_off[map] + ((size_t)(px + si) * W + (py + sj)) * a.C;
      lab = a.labels[a.lab_off[map] + (size_t)(px + si) * W + (py + sj)];
    }
    // rotated-in fill is value 0 (+ noise), label 0, mask 0: what ndimage.rotate(cval=0) leaves behind
    const bool noisy = a.noise_on && a.noise_on[b];
    for (int c = 0; c < a.C; ++c) {
      double e = valid ? (double)src[c] : 0.0;      // fp64 until the single rounding on the store
      if (noisy) {
        const size_t ne = (((size_t)b * a.S + fi) * a.S + fj) * a.C + c;   // noise is indexed before the flip
        const size_t ng = ne + (size_t)a.b0 * a.S * a.S * a.C;             // ... and by the patch's place in the GLOBAL batch on the device path
        if (a.noise) e = e + a.noise[ne];
        else {
          unsigned r[4];
          philox(a.seed, (unsigned long long)ng, r);
          e = e + 0.01 * normal_from(r[0], r[1]);
        }
      }
      if (a.quantize_f16) {
        // coffee:293 casts the patches to float16, coffee:67-74 normalises in that array.  NumPy >= 2 (NEP 50) evaluates
        // float16-array (op) numpy-scalar in the SCALAR's type when that is wider, and the assignment rounds to float16:
        // 1 = float32 scalars (what coffee's own compute_image_mean gives: np.mean / np.std of float32 patches), 2 = float64 scalars
        _Float16 q = (_Float16)(float)e;
        if (c < 3) {
          if (a.quantize_f16 == 2) {
            q = (_Float16)((double)q - a.mean[c]);
            q = (_Float16)((double)q / a.stdv[c]);
          } else {
            q = (_Float16)((float)q - (float)a.mean[c]);
            q = (_Float16)((float)q / (float)a.stdv[c]);
          }
        }
        v[c] = (float)q;
        continue;
      }
      if (c < 3) e = (e - a.mean[c]) / a.stdv[c];
      v[c] = (float)e;
    }
    if (a.out_lab) a.out_lab[opix] = lab;
    if (a.out_mask) a.out_mask[opix] = (valid && (int)lab != a.void_label) ? 1 : 0;
  }
  // one pixel = ld floats: the real channels, then zero padding up to the conv1 K-step
  for (int c4 = 0; c4 < a.ld; c4 += 4) {
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (c4 + k) < 8 ? v[(c4 + k) & 7] : 0.f;
    *reinterpret_cast<f32x4*>(dst + c4) = o;
  }
}

// One axis of the scale-jitter crop (include/drs.h, drs_crop_normalize_scaled): patch pixel p of a side-S patch whose footprint has
// the centre c (pixel-edge coordinates) and `step` source pixels per patch pixel, on a map axis of n pixels.  u is the pixel centre's
// position; it is valid iff 0 <= u <= n (a NaN fails both); the bilinear neighbours are those of D (resample_axis), the label's
// source pixel the one that contains u.  Every product and sum is rounded on its own (fp contract(off)).
__device__ __forceinline__ bool jitter_axis(int p, int S, double c, double step, int n, int& i0, int& i1, double& l, int& il) {
  const double t = ((double)p + 0.5) - 0.5 * (double)S;
  const double u = c + t * step;
  if (!(u >= 0.0 && u <= (double)n)) return false;
  double src = u - 0.5;
  if (src < 0.0) src = 0.0;
  if (src > (double)(n - 1)) src = (double)(n - 1);
  i0 = (int)src;
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  l = src - (double)i0;
  il = (int)u;
  if (il > n - 1) il = n - 1;
  return true;
}

// drs_crop_normalize_scaled: crop_kernel for training with scale jitter.  A sibling with a body of its own, not a
// template parameter of crop_kernel: crop_kernel is held to the code it compiled to before this kernel existed (a shared body, even
// with the new branches compiled out, came out scheduled differently), so its text above is left alone and what the two share is
// restated here line by line.  What differs: the patch pixel (si, sj) the rotation picked is resampled from the footprint
// geo[b] = (step, cy, cx) instead of copied from (px + si, py + sj); geo and the map index are device data and are checked here: a bad
// row leaves a zero patch (no noise) with label 0 and mask 0.  Same grid: one thread per slab pixel in store order; four gathered
// source pixels per patch pixel.
template <typename T>
__global__ void crop_scaled_kernel(const CropArgs a, const double* __restrict__ geo, int n_maps) {
  const int Sp = a.S + 2 * a.P;
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= Sp) return;
  const int b = blockIdx.y / Sp, yy = blockIdx.y - b * Sp;
  float* dst = a.out + ((size_t)(b * Sp + yy) * Sp + xx) * a.ld;
  const int i = yy - a.P, j = xx - a.P;
  const bool inside = i >= 0 && i < a.S && j >= 0 && j < a.S;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (inside) {
    const int map = a.inst[4 * b], flip = a.inst[4 * b + 3];     // (row, col are not read: the centre is in geo)
    // undo the flip (applied last by the reference), then the rotation (applied first)
    const int fi = flip == 1 ? a.S - 1 - i : i, fj = flip == 2 ? a.S - 1 - j : j;
    int si = fi, sj = fj;
    bool valid = true;
    if (a.rot_on && a.rot_on[b]) {
      const double* m = a.rot + 6 * b;
      // scipy.ndimage geometric transform, order 0: in = M . out + offset (no FMA contraction), nearest = floor(c + 0.5)
      // (plain operators under this file's `fp contract(off)`: every product and every sum rounded on its own, as in ndimage's C)
      const double p00 = (double)fi * m[0], p01 = (double)fj * m[1], p10 = (double)fi * m[2], p11 = (double)fj * m[3];
      double c0 = 0.0 + p00;
      c0 = c0 + p01;
      c0 = c0 + m[4];
      double c1 = 0.0 + p10;
      c1 = c1 + p11;
      c1 = c1 + m[5];
      valid = !(c0 < 0.0 || c0 > (double)(a.S - 1) || c1 < 0.0 || c1 > (double)(a.S - 1));
      si = (int)floor(c0 + 0.5);
      sj = (int)floor(c1 + 0.5);
    }
    const size_t opix = ((size_t)b * a.S + i) * a.S + j;
    unsigned char lab = 0;
    const T* src = nullptr;
    const T* s01 = nullptr; const T* s10 = nullptr; const T* s11 = nullptr;      // the other three neighbours (src is v00)
    double ly = 0.0, lx = 0.0;
    const double step = geo[3 * b], cy = geo[3 * b + 1], cx = geo[3 * b + 2];
    // the device-side check of geo and the map index (a NaN fails every comparison)
    const bool bad = !(step > 0.0 && step <= DBL_MAX && fabs(cy) <= DBL_MAX && fabs(cx) <= DBL_MAX) || map < 0 || map >= n_maps;
    if (bad) valid = false;
    if (valid) {
      const int H = a.tile_h[map], W = a.tile_w[map];
      int y0, y1, x0, x1, yl, xl;
      valid = jitter_axis(si, a.S, cy, step, H, y0, y1, ly, yl);
      valid = jitter_axis(sj, a.S, cx, step, W, x0, x1, lx, xl) && valid;
      if (valid) {
        const T* base = reinterpret_cast<const T*>(a.tiles) + a.tile_off[map];
        src = base + ((size_t)y0 * W + x0) * a.C;
        s01 = base + ((size_t)y0 * W + x1) * a.C;
        s10 = base + ((size_t)y1 * W + x0) * a.C;
        s11 = base + ((size_t)y1 * W + x1) * a.C;
        lab = a.labels[a.lab_off[map] + (size_t)yl * W + xl];
      }
    }
    // rotated-in fill and the footprint's overhang are value 0 (+ noise), label 0, mask 0; a bad row is 0 without noise
    const bool noisy = a.noise_on && a.noise_on[b];
    for (int c = 0; c < a.C && !bad; ++c) {
      double e = 0.0;                               // fp64 until the single rounding on the store
      if (valid)                                    // D's expression (crop_tiles_kernel), in its order
        e = (1.0 - ly) * ((1.0 - lx) * (double)src[c] + lx * (double)s01[c]) +
            ly * ((1.0 - lx) * (double)s10[c] + lx * (double)s11[c]);
      if (noisy) {
        const size_t ne = (((size_t)b * a.S + fi) * a.S + fj) * a.C + c;   // noise is indexed before the flip
        const size_t ng = ne + (size_t)a.b0 * a.S * a.S * a.C;             // ... and by the patch's place in the GLOBAL batch on the device path
        if (a.noise) e = e + a.noise[ne];
        else {
          unsigned r[4];
          philox(a.seed, (unsigned long long)ng, r);
          e = e + 0.01 * normal_from(r[0], r[1]);
        }
      }
      if (a.quantize_f16) {
        // coffee:293 casts the patches to float16, coffee:67-74 normalises in that array.  NumPy >= 2 (NEP 50) evaluates
        // float16-array (op) numpy-scalar in the SCALAR's type when that is wider, and the assignment rounds to float16:
        // 1 = float32 scalars (what coffee's own compute_image_mean gives: np.mean / np.std of float32 patches), 2 = float64 scalars
        _Float16 q = (_Float16)(float)e;
        if (c < 3) {
          if (a.quantize_f16 == 2) {
            q = (_Float16)((double)q - a.mean[c]);
            q = (_Float16)((double)q / a.stdv[c]);
          } else {
            q = (_Float16)((float)q - (float)a.mean[c]);
            q = (_Float16)((float)q / (float)a.stdv[c]);
          }
        }
        v[c] = (float)q;
        continue;
      }
      if (c < 3) e = (e - a.mean[c]) / a.stdv[c];
      v[c] = (float)e;
    }
    if (a.out_lab) a.out_lab[opix] = lab;
    if (a.out_mask) a.out_mask[opix] = (valid && (int)lab != a.void_label) ? 1 : 0;
  }
  // one pixel = ld floats: the real channels, then zero padding up to the conv1 K-step
  for (int c4 = 0; c4 < a.ld; c4 += 4) {
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (c4 + k) < 8 ? v[(c4 + k) & 7] : 0.f;
    *reinterpret_cast<f32x4*>(dst + c4) = o;
  }
}

// ------------------------------------------------------------------------------------------------ stitch
struct StitchArgs {
  float* prob;            // [h][w][K]
  unsigned int* occur;    // [h][w]   (the reference replicates the count over K; one copy is kept)
  const float* logits;    // [nb][S][S][K]
  int h, w, K, S, stride, n_h, n_w;
  int f0, nb;             // windows f0 .. f0+nb-1 (row-major flat index) are in `logits`
  int row0, nrows;        // image rows touched by this batch
};

// windows along one axis that cover coordinate v, in ascending window index: regular ones at r*stride, plus the
// last one when it was shifted back to end at the border (isprs:366-375)
__device__ __forceinline__ int covering(int v, int len, int S, int stride, int n, int (&idx)[6], int (&pos)[6]) {
  const int n_reg = (len - S) / stride + 1;
  int lo = v - S + 1; lo = lo <= 0 ? 0 : (lo + stride - 1) / stride;
  int hi = v / stride; if (hi > n_reg - 1) hi = n_reg - 1;
  int cnt = 0;
  for (int r = lo; r <= hi && cnt < 5; ++r) { idx[cnt] = r; pos[cnt] = r * stride; ++cnt; }
  if (n > n_reg && v >= len - S) { idx[cnt] = n - 1; pos[cnt] = len - S; ++cnt; }
  return cnt;
}

// one thread per image pixel of the touched band; windows are added in their flat (reference) order
__global__ void stitch_accumulate_kernel(const StitchArgs a) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = a.row0 + blockIdx.y;
  if (x >= a.w || y >= a.h) return;
  int ri[6], rp[6], ci[6], cp[6];
  const int nr = covering(y, a.h, a.S, a.stride, a.n_h, ri, rp);
  const int nc = covering(x, a.w, a.S, a.stride, a.n_w, ci, cp);
  float acc[8];
  float* pp = a.prob + ((size_t)y * a.w + x) * a.K;
  for (int k = 0; k < a.K; ++k) acc[k] = pp[k];
  unsigned cnt = 0;
  for (int i = 0; i < nr; ++i)
    for (int j = 0; j < nc; ++j) {
      const int f = ri[i] * a.n_w + ci[j] - a.f0;
      if (f < 0 || f >= a.nb) continue;
      const float* lg = a.logits + (((size_t)f * a.S + (y - rp[i])) * a.S + (x - cp[j])) * a.K;
      for (int k = 0; k < a.K; ++k) acc[k] += lg[k];
      ++cnt;
    }
  if (cnt) {
    for (int k = 0; k < a.K; ++k) pp[k] = acc[k];
    a.occur[(size_t)y * a.w + x] += cnt;
  }
}

// overlap-tile inference: the core box of tile i, (y0, x0, cy0, cy1, cx0, cx1) = origin and half-open core rows / columns in image
// coordinates, is copied out of the tile's [T][T][K] logits into prob and counted in occur.  One thread per tile pixel; the box is
// checked here (it is device data): a box outside the image or outside its tile places nothing, and the coverage count shows the gap.
struct TilePlaceArgs {
  float* prob;            // [h][w][K]
  unsigned int* occur;    // [h][w]
  const float* logits;    // [n][T][T][K]
  const int* boxes;       // [n][6]
  int h, w, K, T;
};

// the image pixel (y, x) under pixel (ty, tx) of tile i, if it lies in the tile's core: false for a thread past the tile, a box outside
// the image or outside its tile, or a pixel outside the core
__device__ __forceinline__ bool core_pixel(const int* boxes, int i, int ty, int tx, int h, int w, int T, int& y, int& x) {
  if (tx >= T || ty >= T) return false;
  const int* b = boxes + 6 * (size_t)i;
  const int y0 = b[0], x0 = b[1], cy0 = b[2], cy1 = b[3], cx0 = b[4], cx1 = b[5];
  if (y0 < 0 || x0 < 0 || y0 > h - T || x0 > w - T) return false;
  if (cy0 < y0 || cy1 > y0 + T || cy0 > cy1 || cx0 < x0 || cx1 > x0 + T || cx0 > cx1) return false;
  y = y0 + ty;
  x = x0 + tx;
  return y >= cy0 && y < cy1 && x >= cx0 && x < cx1;
}

__global__ void tile_place_kernel(const TilePlaceArgs a) {
  const int i = blockIdx.z, ty = blockIdx.y;
  const int tx = blockIdx.x * blockDim.x + threadIdx.x;
  int y, x;
  if (!core_pixel(a.boxes, i, ty, tx, a.h, a.w, a.T, y, x)) return;
  const float* lg = a.logits + (((size_t)i * a.T + ty) * a.T + tx) * a.K;
  float* pp = a.prob + ((size_t)y * a.w + x) * a.K;
  for (int k = 0; k < a.K; ++k) pp[k] = lg[k];
  atomicAdd(a.occur + (size_t)y * a.w + x, 1u);      // (a plan whose cores overlap counts 2 there, not a lost update)
}

// ------------------------------------------------------------------------------------------------ dihedral test-time augmentation
// A code g in 0..7 is one symmetry of the square (include/drs.h): bit 0 fx (flip columns), bit 1 fy (flip rows), bit 2 t (transpose).
// sigma_g(i, j): flip first, then transpose -- Y[i][j] = X[sigma_g(i, j)];  sigma_g^-1(a, b): transpose first, then flip.
__device__ __forceinline__ void dihedral_fwd(int g, int T, int i, int j, int& si, int& sj) {
  const int fi = (g & 2) ? T - 1 - i : i, fj = (g & 1) ? T - 1 - j : j;
  if (g & 4) { si = fj; sj = fi; } else { si = fi; sj = fj; }
}
__device__ __forceinline__ void dihedral_inv(int g, int T, int a, int b, int& si, int& sj) {
  const int ta = (g & 4) ? b : a, tb = (g & 4) ? a : b;
  si = (g & 2) ? T - 1 - ta : ta;
  sj = (g & 1) ? T - 1 - tb : tb;
}

// the core of tile i (boxes as tile_place_kernel, checked the same way) gets the softmax of the logits the net computed for the
// g-transformed tile, mapped back by sigma_g^-1, ADDED into acc; occur counts.  One thread per tile pixel in image order (coalesced
// read-modify-write of acc); the cores of one plan are disjoint, so the plain read-modify-write is race-free and deterministic.
struct TilePlaceDihedralArgs {
  float* acc;             // [h][w][K]
  unsigned int* occur;    // [h][w]
  const float* logits;    // [n][T][T][K], on the transformed tile's grid
  const int* boxes;       // [n][6]
  int h, w, K, T, g;
};

__global__ void tile_place_dihedral_kernel(const TilePlaceDihedralArgs a) {
  const int i = blockIdx.z, ty = blockIdx.y;
  const int tx = blockIdx.x * blockDim.x + threadIdx.x;
  int y, x;
  if (!core_pixel(a.boxes, i, ty, tx, a.h, a.w, a.T, y, x)) return;
  int si, sj;
  dihedral_inv(a.g, a.T, ty, tx, si, sj);
  const float* lg = a.logits + (((size_t)i * a.T + si) * a.T + sj) * a.K;
  float e[8], mx = lg[0], sum = 0.f;
  for (int k = 1; k < a.K; ++k) mx = fmaxf(mx, lg[k]);
  for (int k = 0; k < a.K; ++k) {
    e[k] = expf(lg[k] - mx);            // max-subtracted: unlike the reference's softmax() (isprs:38-43), on purpose
    sum += e[k];
  }
  float* pp = a.acc + ((size_t)y * a.w + x) * a.K;
  for (int k = 0; k < a.K; ++k) pp[k] += e[k] / sum;
  atomicAdd(a.occur + (size_t)y * a.w + x, 1u);
}

// ------------------------------------------------------------------------------------------- multi-scale test-time augmentation
// One axis of the bilinear resampling D(n -> ns) with half-pixel centres (torch interpolate, bilinear, align_corners=False, no
// antialias): output index d reads source i0, i1 with weight l on i1.  fp64; at ns == n: (d, d, 0) exactly.
__device__ __forceinline__ void resample_axis(int d, int n, int ns, int& i0, int& i1, double& l) {
  double src = ((double)d + 0.5) * ((double)n / (double)ns) - 0.5;
  if (src < 0.0) src = 0.0;
  i0 = (int)src;
  if (i0 > n - 1) i0 = n - 1;
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  l = src - (double)i0;
}

// conv1's haloed slab of the g-transformed T x T tile at (row, col) of map `map` (drs_crop_dihedral), or of that map bilinearly resampled
// to hs x ws (RESAMPLE: drs_crop_resampled; row, col on that grid): the slab pixel's source is permuted by sigma_g; its value is the source
// pixel's, or the bilinear mix of four source pixels in fp64 -- one fused gather: no resized image exists --; then the normalisation of
// crop_kernel without augmentation (fp64 until the one rounding on the store, bands 0..2).  One thread per slab pixel, so the stores are
// coalesced; a transposed code reads its source with a row stride (absorbed by L2 / the Infinity Cache).  inst is device data: a tile
// outside its map or grid, or a map index out of range, leaves that patch's slab all zeros.
struct CropTilesArgs {
  const void* tiles;
  const long long* tile_off;
  const int* tile_h; const int* tile_w;
  int n_maps, C;
  const int* inst;              // [B][3]: map, row, col (on the hs x ws grid with RESAMPLE)
  int hs, ws, g;                // hs, ws: with RESAMPLE only
  double mean[3], stdv[3];
  float* out; int T, P, ld;     // [B][T+2P][T+2P][ld]
};

template <typename Tp, bool RESAMPLE>
__global__ void crop_tiles_kernel(const CropTilesArgs a) {
  const int Tp2 = a.T + 2 * a.P;
  const int xx = blockIdx.x * blockDim.x + threadIdx.x;
  if (xx >= Tp2) return;
  const int b = blockIdx.y / Tp2, yy = blockIdx.y - b * Tp2;
  float* dst = a.out + ((size_t)(b * Tp2 + yy) * Tp2 + xx) * a.ld;
  const int i = yy - a.P, j = xx - a.P;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i >= 0 && i < a.T && j >= 0 && j < a.T) {
    const int map = a.inst[3 * b], row = a.inst[3 * b + 1], col = a.inst[3 * b + 2];
    if (map >= 0 && map < a.n_maps && row >= 0 && col >= 0 &&
        row <= (RESAMPLE ? a.hs : a.tile_h[map]) - a.T && col <= (RESAMPLE ? a.ws : a.tile_w[map]) - a.T) {
      int si, sj;
      dihedral_fwd(a.g, a.T, i, j, si, sj);
      const int h = a.tile_h[map], w = a.tile_w[map];
      const Tp* base = reinterpret_cast<const Tp*>(a.tiles) + a.tile_off[map];
      int y0 = row + si, y1 = y0, x0 = col + sj, x1 = x0;
      double ly = 0.0, lx = 0.0;
      if (RESAMPLE) {
        resample_axis(row + si, h, a.hs, y0, y1, ly);
        resample_axis(col + sj, w, a.ws, x0, x1, lx);
      }
      const Tp* s00 = base + ((size_t)y0 * w + x0) * a.C;
      const Tp* s01 = base + ((size_t)y0 * w + x1) * a.C;
      const Tp* s10 = base + ((size_t)y1 * w + x0) * a.C;
      const Tp* s11 = base + ((size_t)y1 * w + x1) * a.C;
      for (int c = 0; c < a.C; ++c) {
        double e = (double)s00[c];
        if (RESAMPLE)
          e = (1.0 - ly) * ((1.0 - lx) * (double)s00[c] + lx * (double)s01[c]) +
              ly * ((1.0 - lx) * (double)s10[c] + lx * (double)s11[c]);
        if (c < 3) e = (e - a.mean[c]) / a.stdv[c];
        v[c] = (float)e;
      }
    }
  }
  for (int c4 = 0; c4 < a.ld; c4 += 4) {
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (c4 + k) < 8 ? v[(c4 + k) & 7] : 0.f;
    *reinterpret_cast<f32x4*>(dst + c4) = o;
  }
}

// the class-probability vector of one pixel from its K accumulated values s and its divisor oc: s / oc (a probability sum,
// src_is_prob) or the max-subtracted softmax of s / oc (logits), written as in tile_place_dihedral_kernel.  For logits mx is the
// largest quotient and the return value the sum of the exponentials (what the entropy of score_maps_kernel is made of); for
// probabilities mx is not set and the return value is 0.
__device__ __forceinline__ float prob_from_sums(const float* s, float oc, int K, int src_is_prob, float* p, float& mx) {
  if (src_is_prob) {
    for (int k = 0; k < K; ++k) p[k] = s[k] / oc;
    return 0.f;
  }
  mx = s[0] / oc;
  float sum = 0.f;
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, s[k] / oc);
  for (int k = 0; k < K; ++k) {
    p[k] = expf(s[k] / oc - mx);
    sum += p[k];
  }
  for (int k = 0; k < K; ++k) p[k] = p[k] / sum;
  return sum;
}

// the class-probability vector of pixel q of an hs x ws map: prob_from_sums of src[q] and occur[q]; occur 0 counts as 1
__device__ __forceinline__ void prob_vector(const float* src, const unsigned int* occur, size_t q, int K, int src_is_prob, float* p) {
  const unsigned int o = occur[q];
  float mx = 0.f;
  prob_from_sums(src + q * K, (float)(o ? o : 1u), K, src_is_prob, p, mx);
}

// acc[h][w][K] += U(hs x ws -> h x w) of the probability vectors: one thread per output pixel in image order (coalesced
// read-modify-write of acc); weights in fp64, rounded once, the four vectors mixed in fp32 in the order of include/drs.h
__global__ void resample_accumulate_kernel(const float* __restrict__ src, const unsigned int* __restrict__ occur, int hs, int ws, int K,
                                           int src_is_prob, int h, int w, float* __restrict__ acc) {
  const int y = blockIdx.y, x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= w || y >= h) return;
  int y0, y1, x0, x1;
  double ly, lx;
  resample_axis(y, hs, h, y0, y1, ly);
  resample_axis(x, ws, w, x0, x1, lx);
  const float wy0 = (float)(1.0 - ly), wy1 = (float)ly, wx0 = (float)(1.0 - lx), wx1 = (float)lx;
  float p00[8], p01[8], p10[8], p11[8];
  prob_vector(src, occur, (size_t)y0 * ws + x0, K, src_is_prob, p00);
  prob_vector(src, occur, (size_t)y0 * ws + x1, K, src_is_prob, p01);
  prob_vector(src, occur, (size_t)y1 * ws + x0, K, src_is_prob, p10);
  prob_vector(src, occur, (size_t)y1 * ws + x1, K, src_is_prob, p11);
  float* pp = acc + ((size_t)y * w + x) * K;
  for (int k = 0; k < K; ++k) pp[k] += wy0 * (wx0 * p00[k] + wx1 * p01[k]) + wy1 * (wx0 * p10[k] + wx1 * p11[k]);
}

// arg-max over classes of prob / max(occur, 1) (first maximum); the division is by a per-pixel positive constant
__global__ void stitch_finalize_kernel(const float* __restrict__ prob, const unsigned int* __restrict__ occur, size_t npix, int K,
                                       unsigned char* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned oc = occur[i] ? occur[i] : 1u;
    int am = 0;
    double best = (double)prob[i * K] / (double)oc;
    for (int k = 1; k < K; ++k) {
      const double v = (double)prob[i * K + k] / (double)oc;
      if (v > best) { best = v; am = k; }
    }
    out[i] = (unsigned char)am;
  }
}

// a score in [0, 1] as a byte: clamped (a NaN counts as 0), then rounded half up on the 255 scale
__device__ __forceinline__ unsigned char score_byte(float s) {
  s = s > 0.f ? (s < 1.f ? s : 1.f) : 0.f;
  return (unsigned char)(int)(255.f * s + 0.5f);
}

// The three blocks drs_stitch_finalize_scores' two kernels share.  score_label: the first maximum of the fp64 quotients s[k] / oc,
// stitch_finalize_kernel's expression.
template <int K>
__device__ __forceinline__ int score_label(const float (&s)[K], unsigned oc) {
  int am = 0;
  double best = (double)s[0] / (double)oc;
#pragma unroll
  for (int k = 1; k < K; ++k) {
    const double v = (double)s[k] / (double)oc;
    if (v > best) { best = v; am = k; }
  }
  return am;
}

// no window or tile reached pixel i: nothing is known about it
__device__ __forceinline__ void score_uncovered(size_t i, unsigned char* confidence, unsigned char* margin, unsigned char* entropy) {
  if (confidence) confidence[i] = 0;
  if (margin) margin[i] = 0;
  if (entropy) entropy[i] = 255;
}

// the bytes of pixel i from its probability vector p, its label am and its normalised entropy hn (formed by the caller, and only where
// that map is asked for): confidence p[am], margin p[am] - the largest other p, entropy hn
template <int K>
__device__ __forceinline__ void score_write(size_t i, const float (&p)[K], int am, float hn, unsigned char* confidence,
                                            unsigned char* margin, unsigned char* entropy) {
  float top = p[0], second = 0.f;
#pragma unroll
  for (int k = 1; k < K; ++k) top = k == am ? p[k] : top;
  bool first = true;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (k == am) continue;
    second = first ? p[k] : fmaxf(second, p[k]);
    first = false;
  }
  if (confidence) confidence[i] = score_byte(top);
  if (margin) margin[i] = score_byte(top - second);
  if (entropy) entropy[i] = score_byte(hn);
}

// drs_stitch_finalize with the per-pixel score maps (include/drs.h: confidence, margin, normalised entropy) beside the label: one
// thread per pixel, grid-stride, the pixel's K sums read once into registers (K is a template parameter: the loops unroll and
// nothing spills).  The label is stitch_finalize_kernel's expression, the probability vector is prob_from_sums'.  Every output is one
// byte per pixel in pixel order, so a wave writes 64 consecutive bytes per map; a NULL map is not computed for, nor written.
template <int K>
__global__ void score_maps_kernel(const float* __restrict__ sums, const unsigned int* __restrict__ occur, size_t npix, int sums_are_prob,
                                  unsigned char* __restrict__ labels, unsigned char* __restrict__ confidence,
                                  unsigned char* __restrict__ margin, unsigned char* __restrict__ entropy) {
  const bool want_scores = confidence || margin || entropy;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned o = occur[i];
    const unsigned oc = o ? o : 1u;
    float s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = sums[i * K + k];
    const int am = score_label<K>(s, oc);
    if (labels) labels[i] = (unsigned char)am;
    if (!want_scores) continue;
    if (!o) {
      score_uncovered(i, confidence, margin, entropy);
      continue;
    }
    const float ocf = (float)oc;
    float p[K], mx = 0.f;
    const float se = prob_from_sums(s, ocf, K, sums_are_prob, p, mx);
    float hn = 0.f;          // one class: the entropy is 0, and so is its normalised form here
    if (entropy && K > 1) {
      float acc = 0.f;
      if (sums_are_prob) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc += p[k] > 0.f ? p[k] * logf(p[k]) : 0.f;      // 0 ln 0 = 0
        hn = -acc / logf((float)K);
      } else {
        // -sum p ln p with ln p_k = (v_k - max) - ln se: no logarithm of an underflowed p_k is formed
#pragma unroll
        for (int k = 0; k < K; ++k) acc += p[k] * (s[k] / ocf - mx);
        hn = (logf(se) - acc) / logf((float)K);
      }
    }
    score_write<K>(i, p, am, hn, confidence, margin, entropy);
  }
}

// score_maps_kernel at an inverse temperature beta != 1 (include/drs.h: drs_stitch_finalize_scores_t): a sibling
// kernel, so that score_maps_kernel and its register figures stay what they are.  The label is the same expression; the scores are
// of p = softmax(beta v), v the quotients (logits) or the logarithm of the quotients clamped at FLT_MIN (probabilities).  t = beta v
// is rounded to fp32 before the maximum is subtracted (__fmul_rn keeps the product out of a fused multiply-subtract), so that the
// kernel's t is the one an fp32 product gives.  Renormalised in both modes; the entropy is the logits' form of score_maps_kernel.
template <int K>
__global__ void score_maps_t_kernel(const float* __restrict__ sums, const unsigned int* __restrict__ occur, size_t npix, int sums_are_prob,
                                    float beta, unsigned char* __restrict__ labels, unsigned char* __restrict__ confidence,
                                    unsigned char* __restrict__ margin, unsigned char* __restrict__ entropy) {
  const bool want_scores = confidence || margin || entropy;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned o = occur[i];
    const unsigned oc = o ? o : 1u;
    float s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = sums[i * K + k];
    const int am = score_label<K>(s, oc);
    if (labels) labels[i] = (unsigned char)am;
    if (!want_scores) continue;
    if (!o) {
      score_uncovered(i, confidence, margin, entropy);
      continue;
    }
    const float ocf = (float)oc;
    float t[K], p[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float q = s[k] / ocf;
      t[k] = __fmul_rn(beta, sums_are_prob ? logf(fmaxf(q, FLT_MIN)) : q);
    }
    float mx = t[0], se = 0.f;
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, t[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      t[k] = t[k] - mx;
      p[k] = expf(t[k]);
      se += p[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] = p[k] / se;
    float hn = 0.f;
    if (entropy && K > 1) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) acc += p[k] * t[k];
      hn = (logf(se) - acc) / logf((float)K);
    }
    score_write<K>(i, p, am, hn, confidence, margin, entropy);
  }
}

// multi-scale evaluation (isprs:1347-1474): per scale, softmax over classes of the averaged logits, summed over scales
__global__ void softmax_accumulate_kernel(const float* __restrict__ prob, const unsigned int* __restrict__ occur, size_t npix, int K,
                                          float* __restrict__ acc) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const double oc = (double)(occur[i] ? occur[i] : 1u);
    float e[8], sum = 0.f;
    for (int k = 0; k < K; ++k) {
      e[k] = expf((float)((double)prob[i * K + k] / oc));     // the reference's softmax() has no max subtraction (isprs:38-43)
      sum += e[k];
    }
    for (int k = 0; k < K; ++k) acc[i * K + k] += e[k] / sum;
  }
}

// drs_crop_dihedral / drs_crop_resampled (RESAMPLE: on the hs x ws grid): the argument checks and the launch
template <bool RESAMPLE>
int launch_crop_tiles(const void* tiles, int tiles_are_f64, const long long* tile_off, const int* tile_h, const int* tile_w, int n_maps, int C,
                      const int* inst, int hs, int ws, int g, const double* mean3, const double* std3, int B, int T, int P, int ld,
                      float* out, void* stream) {
  if (!tiles || !tile_off || !tile_h || !tile_w || !inst || !out || !mean3 || !std3) return DRS_ERR_ARG;
  if (n_maps < 1 || C < 1 || C > 8 || ld < C || ld % 4 || g < 0 || g > 7 || !drs_rows_ok(B, T, P)) return DRS_ERR_ARG;
  if (RESAMPLE && (hs < 1 || ws < 1)) return DRS_ERR_ARG;
  const int Tp2 = T + 2 * P;
  CropTilesArgs a;
  a.tiles = tiles; a.tile_off = tile_off; a.tile_h = tile_h; a.tile_w = tile_w; a.n_maps = n_maps; a.C = C; a.inst = inst;
  a.hs = hs; a.ws = ws; a.g = g;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.stdv[c] = std3[c]; }
  a.out = out; a.T = T; a.P = P; a.ld = ld;
  dim3 grid((Tp2 + 63) / 64, B * Tp2);
  if (tiles_are_f64) DRS_LAUNCH((crop_tiles_kernel<double, RESAMPLE>), grid, dim3(64), 0, (hipStream_t)stream, a);
  else DRS_LAUNCH((crop_tiles_kernel<float, RESAMPLE>), grid, dim3(64), 0, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

// drs_stitch_finalize_scores / drs_stitch_finalize_scores_t (TEMPERED: at the inverse temperature beta): the argument checks, the grid
// and the instantiation for K
template <bool TEMPERED>
int launch_scores(const float* sums, const unsigned int* occur, int h, int w, int K, int sums_are_prob, float beta, unsigned char* labels,
                  unsigned char* confidence, unsigned char* margin, unsigned char* entropy, void* stream) {
  if (!sums || !occur || K < 1 || K > 8 || h < 1 || w < 1) return DRS_ERR_ARG;
  if (!labels && !confidence && !margin && !entropy) return DRS_ERR_ARG;
  const size_t n = (size_t)h * w;
  const size_t nb = (n + 255) / 256;
  const dim3 grid(nb < 4096 ? (unsigned)nb : 4096u);
  const int prob = sums_are_prob ? 1 : 0;
#define DRS_SCORES_CASE(KK)                                                                                                        \
  case KK:                                                                                                                         \
    if (TEMPERED)                                                                                                                  \
      DRS_LAUNCH(score_maps_t_kernel<KK>, grid, dim3(256), 0, (hipStream_t)stream, sums, occur, n, prob, beta, labels, confidence, \
                 margin, entropy);                                                                                                 \
    else                                                                                                                           \
      DRS_LAUNCH(score_maps_kernel<KK>, grid, dim3(256), 0, (hipStream_t)stream, sums, occur, n, prob, labels, confidence, margin, \
                 entropy);                                                                                                         \
    break;
  switch (K) {
    DRS_SCORES_CASE(1) DRS_SCORES_CASE(2) DRS_SCORES_CASE(3) DRS_SCORES_CASE(4)
    DRS_SCORES_CASE(5) DRS_SCORES_CASE(6) DRS_SCORES_CASE(7) DRS_SCORES_CASE(8)
  }
#undef DRS_SCORES_CASE
  return DRS_LAUNCH_CHECK();
}

}  // namespace

extern "C" {

int drs_crop_normalize(const void* tiles, int tiles_are_f64, const unsigned char* labels, const long long* tile_off,
                       const long long* lab_off, const int* tile_h, const int* tile_w, int C, const int* inst,
                       const double* rot, const unsigned char* rot_on, const double* noise, const unsigned char* noise_on,
                       unsigned long long seed, int noise_index0, const double* mean3, const double* std3, int B, int S, int P, int ld,
                       float* out, unsigned char* out_lab, unsigned char* out_mask, int void_label, int quantize_f16, void* stream) {
  if (!tiles || !labels || !tile_off || !lab_off || !tile_h || !tile_w || !inst || !out || !mean3 || !std3) return DRS_ERR_ARG;
  if (C < 1 || C > 8 || ld < C || ld % 4 || !drs_rows_ok(B, S, P) || noise_index0 < 0) return DRS_ERR_ARG;
  if (quantize_f16 < 0 || quantize_f16 > 2) return DRS_ERR_ARG;
  const int Sp = S + 2 * P;
  CropArgs a;
  a.tiles = tiles; a.labels = labels; a.tile_off = tile_off; a.lab_off = lab_off; a.tile_h = tile_h; a.tile_w = tile_w; a.C = C;
  a.inst = inst; a.rot = rot; a.rot_on = rot ? rot_on : nullptr; a.noise = noise; a.noise_on = noise_on; a.seed = seed; a.b0 = noise_index0; a.void_label = void_label; a.quantize_f16 = quantize_f16;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.stdv[c] = std3[c]; }
  a.out = out; a.S = S; a.P = P; a.ld = ld; a.out_lab = out_lab; a.out_mask = out_mask;
  dim3 grid((Sp + 63) / 64, B * Sp);
  if (tiles_are_f64) DRS_LAUNCH(crop_kernel<double>, grid, dim3(64), 0, (hipStream_t)stream, a);
  else DRS_LAUNCH(crop_kernel<float>, grid, dim3(64), 0, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

int drs_crop_normalize_scaled(const void* tiles, int tiles_are_f64, const unsigned char* labels, const long long* tile_off,
                              const long long* lab_off, const int* tile_h, const int* tile_w, int n_maps, int C, const int* inst,
                              const double* geo, const double* rot, const unsigned char* rot_on, const double* noise,
                              const unsigned char* noise_on, unsigned long long seed, int noise_index0, const double* mean3,
                              const double* std3, int B, int S, int P, int ld, float* out, unsigned char* out_lab,
                              unsigned char* out_mask, int void_label, int quantize_f16, void* stream) {
  if (!tiles || !labels || !tile_off || !lab_off || !tile_h || !tile_w || !inst || !geo || !out || !mean3 || !std3) return DRS_ERR_ARG;
  if (n_maps < 1 || C < 1 || C > 8 || ld < C || ld % 4 || !drs_rows_ok(B, S, P) || noise_index0 < 0) return DRS_ERR_ARG;
  if (quantize_f16 < 0 || quantize_f16 > 2) return DRS_ERR_ARG;
  const int Sp = S + 2 * P;
  CropArgs a;
  a.tiles = tiles; a.labels = labels; a.tile_off = tile_off; a.lab_off = lab_off; a.tile_h = tile_h; a.tile_w = tile_w; a.C = C;
  a.inst = inst; a.rot = rot; a.rot_on = rot ? rot_on : nullptr; a.noise = noise; a.noise_on = noise_on; a.seed = seed; a.b0 = noise_index0; a.void_label = void_label; a.quantize_f16 = quantize_f16;
  for (int c = 0; c < 3; ++c) { a.mean[c] = mean3[c]; a.stdv[c] = std3[c]; }
  a.out = out; a.S = S; a.P = P; a.ld = ld; a.out_lab = out_lab; a.out_mask = out_mask;
  dim3 grid((Sp + 63) / 64, B * Sp);
  if (tiles_are_f64) DRS_LAUNCH(crop_scaled_kernel<double>, grid, dim3(64), 0, (hipStream_t)stream, a, geo, n_maps);
  else DRS_LAUNCH(crop_scaled_kernel<float>, grid, dim3(64), 0, (hipStream_t)stream, a, geo, n_maps);
  return DRS_LAUNCH_CHECK();
}

int drs_stitch_accumulate(float* prob, unsigned int* occur, const float* logits, int h, int w, int K, int S, int stride,
                          int first_window, int n_windows, void* stream) {
  if (!prob || !occur || !logits || K < 1 || K > 8 || S < 1 || h < 1 || w < 1 || S > h || S > w || stride < 1) return DRS_ERR_ARG;
  // covering() lists at most 5 regular windows per axis over a coordinate, plus the one shifted back to the border
  if (((long long)S + stride - 1) / stride > 5) return DRS_ERR_ARG;
  if (!drs_prod_below(1LL << 31, {(h - S) / stride + 2, (w - S) / stride + 2})) return DRS_ERR_ARG;        // the flat window index is an int
  StitchArgs a;
  a.prob = prob; a.occur = occur; a.logits = logits; a.h = h; a.w = w; a.K = K; a.S = S; a.stride = stride;
  a.n_h = (h - S) % stride == 0 ? (h - S) / stride + 1 : (h - S) / stride + 2;
  a.n_w = (w - S) % stride == 0 ? (w - S) / stride + 1 : (w - S) / stride + 2;
  if (first_window < 0 || n_windows < 1 || first_window + n_windows > a.n_h * a.n_w) return DRS_ERR_ARG;
  a.f0 = first_window; a.nb = n_windows;
  const int r_first = first_window / a.n_w, r_last = (first_window + n_windows - 1) / a.n_w;
  const int y0 = r_first * stride < h - S ? r_first * stride : h - S;
  const int y1 = (r_last * stride < h - S ? r_last * stride : h - S) + S;
  a.row0 = y0; a.nrows = y1 - y0;
  if (a.nrows > 65535) return DRS_ERR_ARG;       // the touched rows index grid.y
  dim3 grid((w + 255) / 256, a.nrows);
  DRS_LAUNCH(stitch_accumulate_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

int drs_tile_place(float* prob, unsigned int* occur, const float* logits, int h, int w, int K, int T, const int* boxes, int n, void* stream) {
  if (!prob || !occur || !logits || !boxes || K < 1 || K > 8 || T < 1 || T > h || T > w || n < 1 || n > 65535 || T > 65535) return DRS_ERR_ARG;
  TilePlaceArgs a;
  a.prob = prob; a.occur = occur; a.logits = logits; a.boxes = boxes; a.h = h; a.w = w; a.K = K; a.T = T;
  dim3 grid((T + 255) / 256, T, n);
  DRS_LAUNCH(tile_place_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

int drs_crop_dihedral(const void* tiles, int tiles_are_f64, const long long* tile_off, const int* tile_h, const int* tile_w, int n_maps,
                      int C, const int* inst, int g, const double* mean3, const double* std3, int B, int T, int P, int ld, float* out,
                      void* stream) {
  return launch_crop_tiles<false>(tiles, tiles_are_f64, tile_off, tile_h, tile_w, n_maps, C, inst, 0, 0, g, mean3, std3, B, T, P, ld, out,
                                  stream);
}

int drs_tile_place_dihedral(float* acc, unsigned int* occur, const float* logits, int h, int w, int K, int T, const int* boxes, int n,
                            int g, void* stream) {
  if (!acc || !occur || !logits || !boxes || K < 1 || K > 8 || T < 1 || T > h || T > w || n < 1 || n > 65535 || T > 65535) return DRS_ERR_ARG;
  if (g < 0 || g > 7) return DRS_ERR_ARG;
  TilePlaceDihedralArgs a;
  a.acc = acc; a.occur = occur; a.logits = logits; a.boxes = boxes; a.h = h; a.w = w; a.K = K; a.T = T; a.g = g;
  dim3 grid((T + 255) / 256, T, n);
  DRS_LAUNCH(tile_place_dihedral_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return DRS_LAUNCH_CHECK();
}

int drs_crop_resampled(const void* tiles, int tiles_are_f64, const long long* tile_off, const int* tile_h, const int* tile_w, int n_maps,
                       int C, const int* inst, int hs, int ws, int g, const double* mean3, const double* std3, int B, int T, int P, int ld,
                       float* out, void* stream) {
  return launch_crop_tiles<true>(tiles, tiles_are_f64, tile_off, tile_h, tile_w, n_maps, C, inst, hs, ws, g, mean3, std3, B, T, P, ld, out,
                                 stream);
}

int drs_resample_accumulate(const float* src, const unsigned int* occur, int hs, int ws, int K, int src_is_prob, int h, int w, float* acc,
                            void* stream) {
  if (!src || !occur || !acc || K < 1 || K > 8 || hs < 1 || ws < 1 || h < 1 || w < 1 || h > 65535) return DRS_ERR_ARG;
  dim3 grid((w + 255) / 256, h);
  DRS_LAUNCH(resample_accumulate_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, occur, hs, ws, K, src_is_prob, h, w, acc);
  return DRS_LAUNCH_CHECK();
}

int drs_stitch_finalize(const float* prob, const unsigned int* occur, int h, int w, int K, unsigned char* out, void* stream) {
  if (!prob || !occur || !out || K < 1 || K > 8 || h < 1 || w < 1) return DRS_ERR_ARG;
  const size_t n = (size_t)h * w;
  const size_t nb = (n + 255) / 256;
  DRS_LAUNCH(stitch_finalize_kernel, dim3(nb < 4096 ? (unsigned)nb : 4096u), dim3(256), 0, (hipStream_t)stream, prob, occur,
                     n, K, out);
  return DRS_LAUNCH_CHECK();
}

int drs_stitch_finalize_scores(const float* sums, const unsigned int* occur, int h, int w, int K, int sums_are_prob,
                               unsigned char* labels, unsigned char* confidence, unsigned char* margin, unsigned char* entropy,
                               void* stream) {
  return launch_scores<false>(sums, occur, h, w, K, sums_are_prob, 1.0f, labels, confidence, margin, entropy, stream);
}

int drs_stitch_finalize_scores_t(const float* sums, const unsigned int* occur, int h, int w, int K, int sums_are_prob, float beta,
                                 unsigned char* labels, unsigned char* confidence, unsigned char* margin, unsigned char* entropy,
                                 void* stream) {
  if (!(beta >= 1.0f / 64.0f && beta <= 64.0f)) return DRS_ERR_ARG;          // (a NaN fails both comparisons)
  if (beta == 1.0f) return drs_stitch_finalize_scores(sums, occur, h, w, K, sums_are_prob, labels, confidence, margin, entropy, stream);
  return launch_scores<true>(sums, occur, h, w, K, sums_are_prob, beta, labels, confidence, margin, entropy, stream);
}

int drs_softmax_accumulate(const float* prob, const unsigned int* occur, int h, int w, int K, float* acc, void* stream) {
  if (!prob || !occur || !acc || K < 1 || K > 8 || h < 1 || w < 1) return DRS_ERR_ARG;
  const size_t n = (size_t)h * w;
  const size_t nb = (n + 255) / 256;
  DRS_LAUNCH(softmax_accumulate_kernel, dim3(nb < 4096 ? (unsigned)nb : 4096u), dim3(256), 0, (hipStream_t)stream, prob, occur, n, K, acc);
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
