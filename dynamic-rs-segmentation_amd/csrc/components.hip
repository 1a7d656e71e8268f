// Connected components of a whole label map, the sieve round built on them and the object census (opt-in; include/drs.h:
// drs_components, drs_sieve_round, drs_component_census).  tests/sieve_ref.py states the rule in numpy.  Everything is
// integer and every cross-workgroup combination is an integer atomic (min, max, add): every output is exact and independent of tiling
// and scheduling.  Below the census: the match of two labellings of one map and the object table (drs_object_match, drs_object_table;
// DESIGN.md 8a.9; tests/objects_ref.py), held to the same discipline -- its one compare-and-swap loop is a weighted majority vote whose
// outcome, where anything reads it, does not depend on the order of the votes.
//
// Labelling is a block-based union-find (Komura 2015; Playne & Hawick 2018): parent[i] <= i always, a root is a pixel with
// parent[i] == i, a union hangs the larger root under the smaller with one atomicMin and goes on with the value that atomic RETURNED
// if the root had moved meanwhile, so the root of a finished tree is the smallest linear index of its component.
//   1. cc_local_kernel   one workgroup per 32 x 32 tile: union-find in LDS, the tile's trees written flat to label[] (= parent[])
//   2. cc_merge_kernel   one thread per pixel on a tile border: unions across the border on the global parent[], agent-scope atomics only
//   3. cc_flatten_kernel (a LATER launch: the forest is finished) every pixel to its root; the pixels of a tile counted per root in an
//                        LDS hash table, one atomicAdd per (component, tile) into size[root]
//   4. cc_spread_kernel  size[p] = size[label[p]]
// No workgroup waits for another anywhere: every loop ends because parents only decrease.
#include "drs_common.hpp"
#include "../../include/drs.h"

namespace {

constexpr int CC_T = 32;                      // tile side
constexpr int CC_PIX = CC_T * CC_T;           // 1024 pixels of a tile
constexpr int CC_THREADS = 256;
constexpr int CC_PER = CC_PIX / CC_THREADS;   // 4 pixels per thread: tile cells t, t + 256, ...
constexpr int CC_HASH = 2 * CC_PIX;           // slots of the per-tile (root -> count) table: at most 1024 distinct roots, so a probe ends
constexpr int CC_MAX_K = 32;
constexpr int CC_MAX_PIXELS = 1 << 30;
constexpr int CC_CENSUS_GRID = 2048;

// ------------------------------------------------------------------------------------------------------------------ union-find
// SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for the LDS forest of a tile, __HIP_MEMORY_SCOPE_AGENT for the global one, where other workgroups
// (other CUs with their own L1, other XCDs with their own L2) write the same words in the same launch.  Every read is an atomic load
// and every decision rests on what an atomic returned.  A stale value read on the way up is still an ancestor (an earlier parent of
// the same word), so the walk only gets longer; that a root IS a root is decided by the atomicMin alone.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* parent, int a) {
  for (;;) {
    const int n = __hip_atomic_load(parent + a, __ATOMIC_RELAXED, SCOPE);
    if (n == a) return a;
    a = n;
  }
}

template <int SCOPE>
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
  for (;;) {
    a = cc_find<SCOPE>(parent, a);
    b = cc_find<SCOPE>(parent, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(parent + b, a, __ATOMIC_RELAXED, SCOPE);      // b was a root iff old == b
    if (old == b) return;
    b = old;                                  // someone hung b elsewhere first (parent[b] is now min(old, a)): unite a with that tree too
  }
}

struct CcArgs {
  const unsigned char* map;
  int* label;
  unsigned int* size;
  int h, w, conn8, tiles_x;
};

// 1. the tile's components in LDS; label[p] = the linear index of the first pixel (row-major) of p's component INSIDE the tile: tile
// cells and map pixels are ordered alike, so that is the smallest linear index.  size[] is zeroed for launch 3's adds.
__global__ void __launch_bounds__(CC_THREADS) cc_local_kernel(const CcArgs a) {
  __shared__ int par[CC_PIX];
  __shared__ unsigned char byt[CC_PIX];
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * CC_T, x0 = tx * CC_T;
#pragma unroll
  for (int j = 0; j < CC_PER; ++j) {
    const int i = threadIdx.x + j * CC_THREADS, gy = y0 + (i >> 5), gx = x0 + (i & 31);
    byt[i] = gy < a.h && gx < a.w ? a.map[(size_t)gy * a.w + gx] : (unsigned char)0;
    par[i] = i;
  }
  __syncthreads();
  // every pair of neighbours belongs to the one of the two that comes later in row-major order: left, up, and with 8 neighbours the
  // two upper diagonals.  Left, up and upper left of a pixel inside the map are inside it; upper right needs gx + 1 < w.
#pragma unroll
  for (int j = 0; j < CC_PER; ++j) {
    const int i = threadIdx.x + j * CC_THREADS, ly = i >> 5, lx = i & 31;
    if (y0 + ly >= a.h || x0 + lx >= a.w) continue;
    const int b = byt[i];
    if (lx > 0 && byt[i - 1] == b) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - 1);
    if (ly > 0 && byt[i - CC_T] == b) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - CC_T);
    if (a.conn8 && ly > 0) {
      if (lx > 0 && byt[i - CC_T - 1] == b) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - CC_T - 1);
      if (lx < CC_T - 1 && x0 + lx + 1 < a.w && byt[i - CC_T + 1] == b) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i, i - CC_T + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CC_PER; ++j) {
    const int i = threadIdx.x + j * CC_THREADS, gy = y0 + (i >> 5), gx = x0 + (i & 31);
    if (gy >= a.h || gx >= a.w) continue;
    const int r = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, i);
    const size_t g = (size_t)gy * a.w + gx;
    a.label[g] = (y0 + (r >> 5)) * a.w + x0 + (r & 31);
    a.size[g] = 0u;
  }
}

// 2. jobs [0, nrb * w): pixel x of the first row of tile row by + 1 against the row above it; jobs after those: pixel y of the first
// column of tile column bx + 1 against the column left of it.  A diagonal pair that crosses a corner is met twice, which a union
// does not mind.  label[] of launch 1 is read here through agent-scope atomics only.
__global__ void __launch_bounds__(CC_THREADS) cc_merge_kernel(const CcArgs a, long long row_jobs, long long jobs) {
  long long j = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (j >= jobs) return;
  const int w = a.w;
  if (j < row_jobs) {
    const int by = (int)(j / w), x = (int)(j - (long long)by * w);
    const int p = (by + 1) * CC_T * w + x;
    const int b = a.map[p];
    if (a.map[p - w] == b) cc_union<__HIP_MEMORY_SCOPE_AGENT>(a.label, p, p - w);
    if (a.conn8) {
      if (x > 0 && a.map[p - w - 1] == b) cc_union<__HIP_MEMORY_SCOPE_AGENT>(a.label, p, p - w - 1);
      if (x + 1 < w && a.map[p - w + 1] == b) cc_union<__HIP_MEMORY_SCOPE_AGENT>(a.label, p, p - w + 1);
    }
  } else {
    j -= row_jobs;
    const int bx = (int)(j / a.h), y = (int)(j - (long long)bx * a.h);
    const int p = y * w + (bx + 1) * CC_T;
    const int b = a.map[p];
    if (a.map[p - 1] == b) cc_union<__HIP_MEMORY_SCOPE_AGENT>(a.label, p, p - 1);
    if (a.conn8) {
      if (y > 0 && a.map[p - w - 1] == b) cc_union<__HIP_MEMORY_SCOPE_AGENT>(a.label, p, p - w - 1);
      if (y + 1 < a.h && a.map[p + w - 1] == b) cc_union<__HIP_MEMORY_SCOPE_AGENT>(a.label, p, p + w - 1);
    }
  }
}

__device__ __forceinline__ void cc_count(int* key, unsigned int* cnt, int root, unsigned int c) {
  unsigned int s = ((unsigned int)root * 2654435761u) >> 21;             // 11 bits: CC_HASH slots
  for (;;) {
    const int old = atomicCAS(key + s, -1, root);
    if (old == -1 || old == root) break;
    s = (s + 1) & (CC_HASH - 1);
  }
  atomicAdd(cnt + s, c);
}

// 3. The forest is finished and no parent changes any more except to its own root here: a walk that meets a word another workgroup
// has already flattened, or an old copy of it, reads an ancestor either way.  A wave whose 64 pixels share a root counts them at once.
__global__ void __launch_bounds__(CC_THREADS) cc_flatten_kernel(const CcArgs a) {
  __shared__ int key[CC_HASH];
  __shared__ unsigned int cnt[CC_HASH];
  for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS) { key[s] = -1; cnt[s] = 0u; }
  __syncthreads();
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * CC_T, x0 = tx * CC_T;
  for (int j = 0; j < CC_PER; ++j) {
    const int i = threadIdx.x + j * CC_THREADS, gy = y0 + (i >> 5), gx = x0 + (i & 31);
    int r = -1;
    if (gy < a.h && gx < a.w) {
      const int p = gy * a.w + gx;
      r = p;
      for (int n = a.label[r]; n != r; n = a.label[r]) r = n;
      a.label[p] = r;
    }
    const int first = __builtin_amdgcn_readfirstlane(r);
    if (__all(r == first)) {
      if (first >= 0 && (threadIdx.x & 63) == 0) cc_count(key, cnt, first, 64u);
    } else if (r >= 0) {
      cc_count(key, cnt, r, 1u);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS)
    if (key[s] >= 0) atomicAdd(a.size + key[s], cnt[s]);
}

// 4. (a root's size is read, never written, here)
__global__ void __launch_bounds__(CC_THREADS) cc_spread_kernel(const int* label, unsigned int* size, int n) {
  const int p = blockIdx.x * CC_THREADS + threadIdx.x;
  if (p >= n) return;
  const int r = label[p];
  if (r != p) size[p] = size[r];
}

// ------------------------------------------------------------------------------------------------------------------ the sieve round
struct SieveArgs {
  const unsigned char* in;
  unsigned char* out;
  const int* label;
  const unsigned int* size;
  unsigned long long* key;                    // the scratch: the best offer of a small component, at its root; 0 = none
  unsigned int* counters;
  int h, w, K;
  unsigned int min_size[CC_MAX_K];
};

__device__ __forceinline__ void sieve_thresholds(const SieveArgs& a, unsigned int* ms) {
  if (threadIdx.x < CC_MAX_K) ms[threadIdx.x] = (int)threadIdx.x < a.K ? a.min_size[threadIdx.x] : 0u;
  __syncthreads();
}

// the scratch words a round reads are those at the roots: zero exactly them, and the counters
__global__ void __launch_bounds__(CC_THREADS) sieve_init_kernel(const SieveArgs a) {
  const int p = blockIdx.x * CC_THREADS + threadIdx.x;
  if (p < 2) a.counters[p] = 0u;
  if (p < a.h * a.w && a.label[p] == p) a.key[p] = 0ull;
}

// a pixel of a small component offers the largest key among its four neighbours: at most one atomic per pixel, and only the pixels
// on the rim of a small component have any offer
__global__ void __launch_bounds__(CC_THREADS) sieve_vote_kernel(const SieveArgs a) {
  __shared__ unsigned int ms[CC_MAX_K];
  sieve_thresholds(a, ms);
  const int p = blockIdx.x * CC_THREADS + threadIdx.x;
  if (p >= a.h * a.w) return;
  const int b = a.in[p];
  if (b >= a.K || a.size[p] >= ms[b]) return;
  const int y = p / a.w, x = p - y * a.w;
  unsigned long long best = 0ull;
  auto offer = [&](int q) {
    const int c = a.in[q];
    if (c == b || c >= a.K) return;
    const unsigned int s = a.size[q];
    if (s < ms[c]) return;
    const unsigned long long k = ((unsigned long long)s << 8) | (unsigned long long)(255 - c);
    best = k > best ? k : best;
  };
  if (y > 0) offer(p - a.w);
  if (x > 0) offer(p - 1);
  if (x + 1 < a.w) offer(p + 1);
  if (y + 1 < a.h) offer(p + a.w);
  if (best) atomicMax(a.key + a.label[p], best);
}

// every thread reads and writes its own pixel only, so out == in is fine
__global__ void __launch_bounds__(CC_THREADS) sieve_relabel_kernel(const SieveArgs a) {
  __shared__ unsigned int ms[CC_MAX_K];
  __shared__ unsigned int tally[2];
  if (threadIdx.x < 2) tally[threadIdx.x] = 0u;
  sieve_thresholds(a, ms);
  const int p = blockIdx.x * CC_THREADS + threadIdx.x;
  if (p < a.h * a.w) {
    const int b = a.in[p];
    int nb = b;
    if (b < a.K && a.size[p] < ms[b]) {
      const int r = a.label[p];
      const unsigned long long k = a.key[r];
      if (k) nb = 255 - (int)(k & 255ull);
      if (r == p) {
        atomicAdd(&tally[0], 1u);
        if (k) atomicAdd(&tally[1], 1u);
      }
    }
    a.out[p] = (unsigned char)nb;
  }
  __syncthreads();
  if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(a.counters + threadIdx.x, tally[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------------------------ the census
__global__ void __launch_bounds__(CC_THREADS) census_kernel(const unsigned char* map, const int* label, const unsigned int* size, int n,
                                                            int K, unsigned long long* table) {
  __shared__ unsigned int tab[CC_MAX_K * 32];
  for (int j = threadIdx.x; j < K * 32; j += CC_THREADS) tab[j] = 0u;
  __syncthreads();
  for (long long p = (long long)blockIdx.x * CC_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * CC_THREADS) {
    const int b = map[p];
    if (label[p] == (int)p && b < K) atomicAdd(&tab[b * 32 + 31 - __clz(size[p])], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < K * 32; j += CC_THREADS)
    if (tab[j]) atomicAdd(table + j, (unsigned long long)tab[j]);
}

// ------------------------------------------------------------------------------------------------------------------ object match
// Two labellings of one map, (tlabel, tsize) of truth and (plabel, psize) of pred.  A truth object t can only match the predicted
// object that holds more than half of it, so the pair table of the two labellings is never made: t's majority partner is found by a
// weighted Boyer-Moore vote, one 64-bit word (candidate << 32 | count) per truth root.
//   1. om_init_kernel    every vote word, inter[] and cover[] zeroed (the result does not depend on what the scratch held)
//   2. om_vote_kernel    one workgroup per tile: the tile's same-class pairs (tlabel, plabel) and its counted pixels per predicted root
//                        counted in LDS; one atomicAdd per (predicted root, tile) into cover[], one weighted vote per (pair, tile)
//   3. om_count_kernel   (a LATER launch: the votes are final) inter[t] += the tile's pixels of the pair (t, candidate[t])
//   4. om_decide_kernel  one thread per pixel: the test 3 I > |t| + cover(candidate) at the truth roots, match[] and inter[] stored
// Any serialisation of the votes of step 2 is a run of the weighted majority algorithm on the same multiset, so where a partner with
// more than half of the votes exists the word ends holding it, whatever the schedule.  Where none exists the candidate is arbitrary,
// but step 3 counts its intersection exactly, the test of step 4 then fails (it implies I > |t| / 2) and inter is stored as 0: no
// output depends on the schedule.  SCOPE as above: workgroup for the LDS tables, agent for the vote words and the adds that other
// workgroups make in the same launch; the next phase reads them in a later launch.
struct OmArgs {
  const unsigned char* truth;
  const unsigned char* pred;
  const int* tlabel;
  const unsigned int* tsize;
  const int* plabel;
  const unsigned int* psize;
  unsigned long long* vote;                   // the scratch
  int* match;
  unsigned int* inter;
  unsigned int* cover;
  int h, w, K, ignore_label, tiles_x;
};

constexpr unsigned long long OM_EMPTY = ~0ull;

__device__ __forceinline__ bool om_counted(const OmArgs& a, int tb) { return tb != a.ignore_label && tb < a.K; }

// the per-tile (pair -> count) table: at most 1024 distinct pairs in CC_HASH slots, so a probe ends
__device__ __forceinline__ void om_count_pair(unsigned long long* key, unsigned int* cnt, unsigned long long pair, unsigned int c) {
  unsigned int s = (((unsigned int)(pair >> 32) * 2654435761u) ^ ((unsigned int)pair * 2246822519u)) >> 21;
  for (;;) {
    const unsigned long long old = atomicCAS(key + s, OM_EMPTY, pair);
    if (old == OM_EMPTY || old == pair) break;
    s = (s + 1) & (CC_HASH - 1);
  }
  atomicAdd(cnt + s, c);
}

// m votes for p in the word of one truth root.  The decision rests on the value the compare-and-swap returned.
__device__ __forceinline__ void om_vote(unsigned long long* word, unsigned int p, unsigned int m) {
  unsigned long long old = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const unsigned int cand = (unsigned int)(old >> 32), c = (unsigned int)old;
    unsigned long long now;
    if (cand == p) now = ((unsigned long long)p << 32) | (unsigned long long)(c + m);
    else if (c >= m) now = ((unsigned long long)cand << 32) | (unsigned long long)(c - m);
    else now = ((unsigned long long)p << 32) | (unsigned long long)(m - c);
    if (__hip_atomic_compare_exchange_strong(word, &old, now, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
}

__global__ void __launch_bounds__(CC_THREADS) om_init_kernel(const OmArgs a) {
  const int p = blockIdx.x * CC_THREADS + threadIdx.x;
  if (p >= a.h * a.w) return;
  a.vote[p] = 0ull;
  a.inter[p] = 0u;
  a.cover[p] = 0u;
}

// A wave whose 64 pixels agree on the pair, or on the predicted root, counts them at once, as the flatten kernel does.
__global__ void __launch_bounds__(CC_THREADS) om_vote_kernel(const OmArgs a) {
  __shared__ unsigned long long pkey[CC_HASH];
  __shared__ unsigned int pcnt[CC_HASH];
  __shared__ int ckey[CC_HASH];
  __shared__ unsigned int ccnt[CC_HASH];
  for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS) { pkey[s] = OM_EMPTY; pcnt[s] = 0u; ckey[s] = -1; ccnt[s] = 0u; }
  __syncthreads();
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * CC_T, x0 = tx * CC_T;
  for (int j = 0; j < CC_PER; ++j) {
    const int i = threadIdx.x + j * CC_THREADS, gy = y0 + (i >> 5), gx = x0 + (i & 31);
    int cov = -1;                             // the predicted root this pixel adds to the cover of
    unsigned long long pair = OM_EMPTY;       // the same-class pair this pixel belongs to
    if (gy < a.h && gx < a.w) {
      const int p = gy * a.w + gx;
      const int tb = a.truth[p], pb = a.pred[p];
      if (om_counted(a, tb) && pb < a.K) {
        cov = a.plabel[p];
        if (pb == tb) pair = ((unsigned long long)(unsigned int)a.tlabel[p] << 32) | (unsigned long long)(unsigned int)cov;
      }
    }
    const int cov0 = __builtin_amdgcn_readfirstlane(cov);
    if (__all(cov == cov0)) {
      if (cov0 >= 0 && (threadIdx.x & 63) == 0) cc_count(ckey, ccnt, cov0, 64u);
    } else if (cov >= 0) {
      cc_count(ckey, ccnt, cov, 1u);
    }
    const unsigned int lo0 = __builtin_amdgcn_readfirstlane((unsigned int)pair), hi0 = __builtin_amdgcn_readfirstlane((unsigned int)(pair >> 32));
    const unsigned long long pair0 = ((unsigned long long)hi0 << 32) | (unsigned long long)lo0;
    if (__all(pair == pair0)) {
      if (pair0 != OM_EMPTY && (threadIdx.x & 63) == 0) om_count_pair(pkey, pcnt, pair0, 64u);
    } else if (pair != OM_EMPTY) {
      om_count_pair(pkey, pcnt, pair, 1u);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS) {
    if (ckey[s] >= 0) atomicAdd(a.cover + ckey[s], ccnt[s]);
    if (pkey[s] != OM_EMPTY) om_vote(a.vote + (pkey[s] >> 32), (unsigned int)pkey[s], pcnt[s]);
  }
}

// 3. the vote words are read, never written, here
__global__ void __launch_bounds__(CC_THREADS) om_count_kernel(const OmArgs a) {
  __shared__ int key[CC_HASH];
  __shared__ unsigned int cnt[CC_HASH];
  for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS) { key[s] = -1; cnt[s] = 0u; }
  __syncthreads();
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * CC_T, x0 = tx * CC_T;
  for (int j = 0; j < CC_PER; ++j) {
    const int i = threadIdx.x + j * CC_THREADS, gy = y0 + (i >> 5), gx = x0 + (i & 31);
    int r = -1;
    if (gy < a.h && gx < a.w) {
      const int p = gy * a.w + gx;
      const int tb = a.truth[p];
      if (om_counted(a, tb) && a.pred[p] == tb) {
        const int t = a.tlabel[p];
        if ((unsigned int)(a.vote[t] >> 32) == (unsigned int)a.plabel[p]) r = t;
      }
    }
    const int first = __builtin_amdgcn_readfirstlane(r);
    if (__all(r == first)) {
      if (first >= 0 && (threadIdx.x & 63) == 0) cc_count(key, cnt, first, 64u);
    } else if (r >= 0) {
      cc_count(key, cnt, r, 1u);
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < CC_HASH; s += CC_THREADS)
    if (key[s] >= 0) atomicAdd(a.inter + key[s], cnt[s]);
}

// 4. every thread reads and writes its own element of inter[] only.  A candidate is a predicted root or the 0 the word started with:
// below h w either way.
__global__ void __launch_bounds__(CC_THREADS) om_decide_kernel(const OmArgs a) {
  const int p = blockIdx.x * CC_THREADS + threadIdx.x;
  if (p >= a.h * a.w) return;
  int m = -2;
  unsigned int keep = 0u;
  if (a.tlabel[p] == p && om_counted(a, a.truth[p])) {
    const unsigned int cand = (unsigned int)(a.vote[p] >> 32);
    const unsigned long long I = a.inter[p];
    m = -1;
    if (3ull * I > (unsigned long long)a.tsize[p] + (unsigned long long)a.cover[cand]) { m = (int)cand; keep = (unsigned int)I; }
  }
  a.match[p] = m;
  a.inter[p] = keep;
}

// ------------------------------------------------------------------------------------------------------------------ object table
constexpr int OT_ROWS = 4;

__global__ void __launch_bounds__(CC_THREADS) object_table_kernel(const OmArgs a, int n, unsigned long long* table) {
  __shared__ unsigned long long tab[CC_MAX_K * OT_ROWS * 32];
  const int cells = a.K * OT_ROWS * 32;
  for (int j = threadIdx.x; j < cells; j += CC_THREADS) tab[j] = 0ull;
  __syncthreads();
  for (long long q = (long long)blockIdx.x * CC_THREADS + threadIdx.x; q < n; q += (long long)gridDim.x * CC_THREADS) {
    const int p = (int)q;
    const int tb = a.truth[p], pb = a.pred[p];
    if (a.tlabel[p] == p && om_counted(a, tb)) {
      const unsigned int ts = a.tsize[p];
      const int bin = 31 - __clz(ts);
      unsigned long long* row = tab + tb * OT_ROWS * 32;
      atomicAdd(row + bin, 1ull);
      const int m = a.match[p];
      if (m >= 0) {
        const unsigned long long I = a.inter[p], cov = a.cover[m];
        atomicAdd(row + 2 * 32 + bin, 1ull);
        atomicAdd(row + 3 * 32 + bin, (I << 20) / ((unsigned long long)ts + cov - I));
        // a matched predicted object counts whatever its cover: the one the walk over the predicted roots below leaves out is added here
        const unsigned int ps = a.psize[m];
        if (2ull * cov < (unsigned long long)ps) atomicAdd(row + 32 + 31 - __clz(ps), 1ull);
      }
    }
    if (a.plabel[p] == p && pb < a.K) {
      const unsigned int ps = a.psize[p];
      if (2ull * (unsigned long long)a.cover[p] >= (unsigned long long)ps) atomicAdd(tab + (pb * OT_ROWS + 1) * 32 + 31 - __clz(ps), 1ull);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < cells; j += CC_THREADS)
    if (tab[j]) atomicAdd(table + j, tab[j]);
}

bool cc_shape_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)h * (long long)w <= (long long)CC_MAX_PIXELS; }

unsigned cc_blocks(long long n) { return (unsigned)((n + CC_THREADS - 1) / CC_THREADS); }

}  // namespace

extern "C" {

int drs_components(const unsigned char* map, int h, int w, int connectivity, int* label, unsigned int* size, void* stream) {
  if (!map || !label || !size || !cc_shape_ok(h, w) || (connectivity != 4 && connectivity != 8)) return DRS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  CcArgs a = {map, label, size, h, w, connectivity == 8 ? 1 : 0, (w + CC_T - 1) / CC_T};
  const int tiles_y = (h + CC_T - 1) / CC_T;
  const unsigned ntiles = (unsigned)a.tiles_x * (unsigned)tiles_y;       // at most 2^25 + (tiles_x + tiles_y): far below the grid limit
  DRS_LAUNCH(cc_local_kernel, dim3(ntiles), dim3(CC_THREADS), 0, st, a);
  int rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  const long long row_jobs = (long long)(tiles_y - 1) * w, jobs = row_jobs + (long long)(a.tiles_x - 1) * h;
  if (jobs > 0) {
    DRS_LAUNCH(cc_merge_kernel, dim3(cc_blocks(jobs)), dim3(CC_THREADS), 0, st, a, row_jobs, jobs);
    rc = DRS_LAUNCH_CHECK();
    if (rc != DRS_OK) return rc;
  }
  DRS_LAUNCH(cc_flatten_kernel, dim3(ntiles), dim3(CC_THREADS), 0, st, a);
  rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(cc_spread_kernel, dim3(cc_blocks((long long)h * w)), dim3(CC_THREADS), 0, st, (const int*)label, size, h * w);
  return DRS_LAUNCH_CHECK();
}

size_t drs_sieve_scratch_bytes(int h, int w) { return cc_shape_ok(h, w) ? (size_t)h * (size_t)w * sizeof(unsigned long long) : 0; }

int drs_sieve_round(const unsigned char* map_in, const int* label, const unsigned int* size, int h, int w, int K, const int* min_size,
                    void* scratch, unsigned char* map_out, unsigned int* counters, void* stream) {
  if (!map_in || !label || !size || !min_size || !scratch || !map_out || !counters || !cc_shape_ok(h, w) || K < 1 || K > CC_MAX_K)
    return DRS_ERR_ARG;
  SieveArgs a = {};
  for (int k = 0; k < K; ++k) {
    if (min_size[k] < 0 || min_size[k] > CC_MAX_PIXELS) return DRS_ERR_ARG;
    a.min_size[k] = (unsigned int)min_size[k];
  }
  a.in = map_in;
  a.out = map_out;
  a.label = label;
  a.size = size;
  a.key = (unsigned long long*)scratch;
  a.counters = counters;
  a.h = h;
  a.w = w;
  a.K = K;
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = cc_blocks((long long)h * w);
  DRS_LAUNCH(sieve_init_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, a);
  int rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(sieve_vote_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, a);
  rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(sieve_relabel_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, a);
  return DRS_LAUNCH_CHECK();
}

int drs_component_census(const unsigned char* map, const int* label, const unsigned int* size, int h, int w, int K,
                         unsigned long long* table, void* stream) {
  if (!map || !label || !size || !table || !cc_shape_ok(h, w) || K < 1 || K > CC_MAX_K) return DRS_ERR_ARG;
  const unsigned need = cc_blocks((long long)h * w);
  DRS_LAUNCH(census_kernel, dim3(need < (unsigned)CC_CENSUS_GRID ? need : (unsigned)CC_CENSUS_GRID), dim3(CC_THREADS), 0,
             (hipStream_t)stream, map, label, size, h * w, K, table);
  return DRS_LAUNCH_CHECK();
}

size_t drs_object_scratch_bytes(int h, int w) { return cc_shape_ok(h, w) ? (size_t)h * (size_t)w * sizeof(unsigned long long) : 0; }

int drs_object_match(const unsigned char* truth, const unsigned char* pred, const int* tlabel, const unsigned int* tsize, const int* plabel,
                     const unsigned int* psize, int h, int w, int K, int ignore_label, void* scratch, int* match, unsigned int* inter,
                     unsigned int* cover, void* stream) {
  if (!truth || !pred || !tlabel || !tsize || !plabel || !psize || !scratch || !match || !inter || !cover || !cc_shape_ok(h, w) || K < 1 ||
      K > CC_MAX_K || ignore_label < -1 || ignore_label > 255)
    return DRS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const OmArgs a = {truth, pred, tlabel, tsize, plabel, psize, (unsigned long long*)scratch, match, inter, cover,
                    h,     w,    K,      ignore_label, (w + CC_T - 1) / CC_T};
  const unsigned ntiles = (unsigned)a.tiles_x * (unsigned)((h + CC_T - 1) / CC_T);
  const unsigned blocks = cc_blocks((long long)h * w);
  DRS_LAUNCH(om_init_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, a);
  int rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(om_vote_kernel, dim3(ntiles), dim3(CC_THREADS), 0, st, a);
  rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(om_count_kernel, dim3(ntiles), dim3(CC_THREADS), 0, st, a);
  rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  DRS_LAUNCH(om_decide_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, a);
  return DRS_LAUNCH_CHECK();
}

int drs_object_table(const unsigned char* truth, const int* tlabel, const unsigned int* tsize, const unsigned char* pred, const int* plabel,
                     const unsigned int* psize, const int* match, const unsigned int* inter, const unsigned int* cover, int h, int w, int K,
                     int ignore_label, unsigned long long* table, void* stream) {
  if (!truth || !tlabel || !tsize || !pred || !plabel || !psize || !match || !inter || !cover || !table || !cc_shape_ok(h, w) || K < 1 ||
      K > CC_MAX_K || ignore_label < -1 || ignore_label > 255)
    return DRS_ERR_ARG;
  const OmArgs a = {truth, pred, tlabel, tsize, plabel, psize, nullptr, const_cast<int*>(match), const_cast<unsigned int*>(inter),
                    const_cast<unsigned int*>(cover), h, w, K, ignore_label, (w + CC_T - 1) / CC_T};
  const unsigned need = cc_blocks((long long)h * w);
  DRS_LAUNCH(object_table_kernel, dim3(need < (unsigned)CC_CENSUS_GRID ? need : (unsigned)CC_CENSUS_GRID), dim3(CC_THREADS), 0,
             (hipStream_t)stream, a, h * w, table);
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
