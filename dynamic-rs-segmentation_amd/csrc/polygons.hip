// Polygon outlines of a whole label map (opt-in; include/drs.h: drs_polygon_count, drs_polygon_rings, drs_polygon_write; DESIGN.md
// 8a.12).  tests/polygon_ref.py states the rule in numpy.  The boundary cracks of the map form disjoint cycles under a local successor
// rule; a ring is such a cycle.  Everything is integer, every combination across workgroups is an integer atomic (add, or) or a scan
// whose partial sums are combined in a fixed order: every output is exact and independent of tiling and scheduling.
//
//   1. pg_mask_kernel      per pixel the 4-bit mask of its cracks and their number
//   2. scan (below)        exclusive scan of the numbers: a crack's SLOT is its pixel's scan value + the cracks of the pixel before
//                          it, so slots are in crack-id order and the slot of any (pixel, side) is computed, never searched
//   3. pg_build_kernel     per crack: id, turn flag, successor slot; the state of the first doubling
//   4. pg_min_round_kernel pointer doubling, (next, min) -> (next of next, min of both) in one 64-bit word per crack: the ring's
//                          leader = its smallest slot
//   5. pg_cut_kernel       every cycle cut in front of its leader: a list that ends at the crack before the leader; the crack's term
//                          of the doubled area added onto the leader's word (one 64-bit integer atomic)
//   6. pg_rank_round_kernel pointer doubling on the lists, suffix sums of (cracks, vertices) in one 16-byte word per crack: a crack's
//                          distance to the list's end
//   7. pg_ringkey_kernel + scan   (1, vertices of the ring) at the leaders, scanned in slot order: ring number and first vertex
//   8. pg_table_kernel     the ring table, one row per leader, in the scratch; pg_finish_kernel stores the counters
// drs_polygon_write then copies the rows and writes every turn crack's head at (first vertex of its ring + its ordinal).
//
// The doubling rounds are launched a fixed number of times, ceil(log2(crack_cap)) (+ 1 for the lists), and ping-pong between two
// buffers: a round reads only what the previous one wrote.  A round that changed nothing leaves a zero flag, the launches after it
// return at once, and the number of rounds run -- kept in the header -- says which buffer holds the result.  No workgroup waits for
// another anywhere, and no loop's length depends on the data.  The successor is computed from the map alone, so it is a bijection on
// the cracks whatever `label` holds.
#include "drs_common.hpp"
#include "../../include/drs.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int PG_THREADS = 256;
constexpr int PG_PER = 4;
constexpr int PG_TILE = PG_THREADS * PG_PER;      // elements of one scan block
constexpr long long PG_MAX_PIXELS = 1LL << 28;    // 4 h w <= 2^30: a crack id and a slot fit in int32; a pixel index divides in 32 bits
constexpr int PG_MAX_ROUNDS = 32;                 // ceil(log2(2^30)) + 1 = 31 rounds at the most
constexpr u32 PG_NIL = 0xffffffffu;
constexpr u32 PG_TURN = 0x80000000u;              // in eid[]: the successor leaves in another direction, the crack's head is a vertex

// the header: the first words of the scratch
enum {
  PG_H_CRACKS = 0,      // the map's crack count (the total of scan 2)
  PG_H_RINGTOTAL,       // rings << 32 | vertices (the total of scan 7)
  PG_H_RINGS,
  PG_H_VERTICES,
  PG_H_STATUS,          // 1: cracks > crack_cap, nothing else in the scratch means anything
  PG_H_SHAPE,           // h << 32 | w of the finished call
  PG_H_CAP,             // crack_cap of the finished call
  PG_H_ROUNDS_MIN,      // rounds of doubling 4 that ran
  PG_H_ROUNDS_RANK,     // rounds of doubling 6 that ran
  PG_H_FLAG_MIN,        // PG_MAX_ROUNDS words: round r changed something
  PG_H_FLAG_RANK = PG_H_FLAG_MIN + PG_MAX_ROUNDS,
  PG_H_WORDS = PG_H_FLAG_RANK + PG_MAX_ROUNDS
};

struct PgLayout {
  size_t pixoff, mask, psum1, psum2, eid, succ, leader, rank[2], a2, scan, ssum1, ssum2, table, bytes;
  long long ring_rows;
};

size_t pg_up(size_t v) { return (v + 255) & ~(size_t)255; }
long long pg_blocks_of(long long n) { return (n + PG_TILE - 1) / PG_TILE; }

// offsets of everything in the scratch.  A ring has at least 4 cracks, so cap / 4 rows hold every ring table.
PgLayout pg_layout(long long n, long long cap) {
  PgLayout L;
  size_t o = pg_up(PG_H_WORDS * sizeof(u64));
  auto take = [&](size_t bytes) { const size_t at = o; o = pg_up(o + bytes); return at; };
  const long long pb1 = pg_blocks_of(n), pb2 = pg_blocks_of(pb1), sb1 = pg_blocks_of(cap), sb2 = pg_blocks_of(sb1);
  L.pixoff = take((size_t)n * 4);
  L.mask = take((size_t)n);
  L.psum1 = take((size_t)pb1 * 4);
  L.psum2 = take((size_t)pb2 * 4);
  L.eid = take((size_t)cap * 4);
  L.succ = take((size_t)cap * 4);
  L.leader = take((size_t)cap * 4);
  L.rank[0] = take((size_t)cap * 16);
  L.rank[1] = take((size_t)cap * 16);      // the words of doubling 4 live here: two 64-bit runs of cap, dead before round 0 of 6
  L.a2 = take((size_t)cap * 8);
  L.scan = take((size_t)cap * 8);
  L.ssum1 = take((size_t)sb1 * 8);
  L.ssum2 = take((size_t)sb2 * 8);
  L.ring_rows = cap / 4;
  L.table = take((size_t)(L.ring_rows > 0 ? L.ring_rows : 1) * 7 * 8);
  L.bytes = o;
  return L;
}

// ------------------------------------------------------------------------------------------------------------------ the scan
// Exclusive scan of n elements in place, three launches per level and no waiting: per-block sums, the scan of those (one level down),
// then every block scans its PG_TILE elements from its offset.  limit (or NULL): a device word; elements from *limit on count as 0 and
// are not written.  With PG_TILE = 1024 and n <= 2^30 there are at most three levels.
template <class T>
__device__ __forceinline__ T pg_block_exclusive(T v, T* lds, T& total) {
  // inclusive scan of the 256 per-thread sums through LDS (Hillis-Steele, 8 steps)
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = 1; s < PG_THREADS; s <<= 1) {
    const T add = t >= s ? lds[t - s] : (T)0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  total = lds[PG_THREADS - 1];
  const T ex = lds[t] - v;
  __syncthreads();
  return ex;
}

__device__ __forceinline__ long long pg_limit(const u64* limit, long long n) {
  if (!limit) return n;
  const u64 l = *limit;
  return l < (u64)n ? (long long)l : n;
}

template <class T>
__global__ void __launch_bounds__(PG_THREADS) pg_scan_sums_kernel(const T* data, long long n, const u64* limit, T* sums) {
  __shared__ T lds[PG_THREADS];
  const long long m = pg_limit(limit, n), base = (long long)blockIdx.x * PG_TILE + (long long)threadIdx.x * PG_PER;
  T v = 0;
#pragma unroll
  for (int j = 0; j < PG_PER; ++j)
    if (base + j < m) v += data[base + j];
  T total;
  pg_block_exclusive<T>(v, lds, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// offsets: the scanned block sums, or NULL for a single block; total_out (or NULL): where a single block stores the grand total
template <class T>
__global__ void __launch_bounds__(PG_THREADS) pg_scan_apply_kernel(T* data, long long n, const u64* limit, const T* offsets, u64* total_out) {
  __shared__ T lds[PG_THREADS];
  const long long m = pg_limit(limit, n), base = (long long)blockIdx.x * PG_TILE + (long long)threadIdx.x * PG_PER;
  T x[PG_PER];
  T v = 0;
#pragma unroll
  for (int j = 0; j < PG_PER; ++j) {
    x[j] = base + j < m ? data[base + j] : (T)0;
    v += x[j];
  }
  T total;
  T run = pg_block_exclusive<T>(v, lds, total) + (offsets ? offsets[blockIdx.x] : (T)0);
#pragma unroll
  for (int j = 0; j < PG_PER; ++j) {
    if (base + j < m) data[base + j] = run;
    run += x[j];
  }
  if (total_out && threadIdx.x == 0) *total_out = (u64)total;
}

template <class T>
int pg_scan(T* data, long long n, const u64* limit, T* sums1, T* sums2, u64* total_out, hipStream_t st) {
  const long long b0 = pg_blocks_of(n);
  int rc;
  if (b0 == 1) {
    DRS_LAUNCH(pg_scan_apply_kernel<T>, dim3(1), dim3(PG_THREADS), 0, st, data, n, limit, (const T*)nullptr, total_out);
    return DRS_LAUNCH_CHECK();
  }
  DRS_LAUNCH(pg_scan_sums_kernel<T>, dim3((unsigned)b0), dim3(PG_THREADS), 0, st, (const T*)data, n, limit, sums1);
  if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  const long long b1 = pg_blocks_of(b0);
  if (b1 == 1) {
    DRS_LAUNCH(pg_scan_apply_kernel<T>, dim3(1), dim3(PG_THREADS), 0, st, sums1, b0, (const u64*)nullptr, (const T*)nullptr, total_out);
    if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  } else {                                   // b1 <= 1024: the third level is one block
    DRS_LAUNCH(pg_scan_sums_kernel<T>, dim3((unsigned)b1), dim3(PG_THREADS), 0, st, (const T*)sums1, b0, (const u64*)nullptr, sums2);
    if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
    DRS_LAUNCH(pg_scan_apply_kernel<T>, dim3(1), dim3(PG_THREADS), 0, st, sums2, b1, (const u64*)nullptr, (const T*)nullptr, total_out);
    if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
    DRS_LAUNCH(pg_scan_apply_kernel<T>, dim3((unsigned)b1), dim3(PG_THREADS), 0, st, sums1, b0, (const u64*)nullptr, (const T*)sums2, (u64*)nullptr);
    if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  }
  DRS_LAUNCH(pg_scan_apply_kernel<T>, dim3((unsigned)b0), dim3(PG_THREADS), 0, st, data, n, limit, (const T*)sums1, (u64*)nullptr);
  return DRS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------------------------ cracks
// side d of pixel (y, x): bit d of the mask is set iff the pixel across it is outside the map or carries another byte
__device__ __forceinline__ u32 pg_mask_of(const unsigned char* map, int h, int w, int y, int x) {
  const size_t p = (size_t)y * w + x;
  const int b = map[p];
  u32 m = 0;
  if (y == 0 || map[p - w] != b) m |= 1u;
  if (x == w - 1 || map[p + 1] != b) m |= 2u;
  if (y == h - 1 || map[p + w] != b) m |= 4u;
  if (x == 0 || map[p - 1] != b) m |= 8u;
  return m;
}

__global__ void __launch_bounds__(PG_THREADS) pg_zero_kernel(u64* words, int n) {
  if ((int)threadIdx.x < n) words[threadIdx.x] = 0ull;
}

__global__ void __launch_bounds__(PG_THREADS) pg_count_kernel(const unsigned char* map, int h, int w, u64* counter) {
  __shared__ u32 lds[PG_THREADS];
  const long long n = (long long)h * w;
  u32 v = 0;
  for (long long p = (long long)blockIdx.x * PG_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * PG_THREADS) {
    const int y = (int)((u32)p / (u32)w), x = (int)p - y * w;
    v += (u32)__popc(pg_mask_of(map, h, w, y, x));
  }
  u32 total;
  pg_block_exclusive<u32>(v, lds, total);
  if (threadIdx.x == 0 && total) atomicAdd(counter, (u64)total);
}

struct PgArgs {
  const unsigned char* map;
  const int* label;
  u64* hdr;
  u32* pixoff;
  unsigned char* mask;
  u32* eid;
  u32* succ;
  u32* leader;
  u64* lead[2];         // doubling 4: next slot << 32 | smallest slot so far -- one word, so that a round gathers once per crack
  uint4* rank[2];       // doubling 6: (next slot or PG_NIL, cracks, vertices from here to the list's end, 0) -- likewise
  u64* a2;
  u64* scan;
  long long* table;
  int h, w, conn8;
  long long cap, ring_rows;
};

__device__ __forceinline__ bool pg_live(const PgArgs& a, long long& count) {
  count = (long long)a.hdr[PG_H_CRACKS];
  return count <= a.cap;
}

__global__ void __launch_bounds__(PG_THREADS) pg_mask_kernel(const PgArgs a) {
  const long long p = (long long)blockIdx.x * PG_THREADS + threadIdx.x;
  if (p >= (long long)a.h * a.w) return;
  const int y = (int)((u32)p / (u32)a.w), x = (int)p - y * a.w;
  const u32 m = pg_mask_of(a.map, a.h, a.w, y, x);
  a.mask[p] = (unsigned char)m;
  a.pixoff[p] = (u32)__popc(m);
}

// the slot of side d of pixel p, a crack
__device__ __forceinline__ u32 pg_slot(const PgArgs& a, long long p, int d) {
  return a.pixoff[p] + (u32)__popc((u32)a.mask[p] & ((1u << d) - 1u));
}

// 3. one thread per pixel, its up to four cracks
__global__ void __launch_bounds__(PG_THREADS) pg_build_kernel(const PgArgs a) {
  long long count;
  if (!pg_live(a, count)) return;
  const long long p = (long long)blockIdx.x * PG_THREADS + threadIdx.x;
  if (p >= (long long)a.h * a.w) return;
  const u32 m = a.mask[p];
  if (!m) return;
  const int h = a.h, w = a.w;
  const int y = (int)((u32)p / (u32)w), x = (int)p - y * w;
  const int b = a.map[p];
  u32 slot = a.pixoff[p];
  const int dx[4] = {1, 0, -1, 0}, dy[4] = {0, 1, 0, -1};
  auto same = [&](int yy, int xx) { return yy >= 0 && yy < h && xx >= 0 && xx < w && a.map[(size_t)yy * w + xx] == b; };
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (!(m >> d & 1u)) continue;
    const int l = (d + 3) & 3;                                   // the side of travel's left: the pixel across side d lies that way
    const int qy = y + dy[d], qx = x + dx[d], ry = qy + dy[l], rx = qx + dx[l];
    const bool sq = same(qy, qx), sr = same(ry, rx);
    // 4: straight on needs q, the left turn q and r; 8: the diagonal pixel r alone makes the left turn
    const bool left = a.conn8 ? sr : sq && sr, straight = !left && sq;
    int ny = y, nx = x, nd = (d + 1) & 3;                        // the right turn: the next side of the same pixel
    if (left) { ny = ry; nx = rx; nd = l; }
    else if (straight) { ny = qy; nx = qx; nd = d; }
    const u32 s = pg_slot(a, (long long)ny * w + nx, nd);
    a.eid[slot] = (u32)(4 * p + d) | (nd != d ? PG_TURN : 0u);
    a.succ[slot] = s;
    a.lead[0][slot] = ((u64)s << 32) | (u64)slot;
    a.a2[slot] = 0ull;
    ++slot;
  }
}

// One vote per workgroup (every thread of the block gets here), and an atomic only while the flag still reads 0: a word that half a
// million waves OR into in one launch serialises them all at its L2 channel.  The build that voted per wave is traced in
// profiles/polygons/kernel_stats_flag_per_wave.csv: rounds of up to 6.0 ms on 34 M cracks, 1182 ms in the two doubling kernels over the
// run; the same run of this build, kernel_stats.csv beside it: rounds of up to 0.31 ms, 122 ms over the run.
__device__ __forceinline__ void pg_flag(u64* flag, bool changed) {
  if (__syncthreads_or(changed) && threadIdx.x == 0 && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull)
    atomicOr(flag, 1ull);
}

// 4. round r: the words of buffer r & 1 -> buffer (r + 1) & 1.  After r rounds min[i] covers the window of the 2^r cracks from i on.
// WHY A ROUND THAT CHANGES NO MIN MAY END THE DOUBLING: nothing changed means min[i] <= min[i + 2^r] for every i (steps along succ).
// Follow one ring from i in steps of 2^r: i, i + 2^r, i + 2 2^r, ... comes back to i, with values that never decrease on the way, so
// they are all equal; and the windows of that orbit lie end to end -- [i + k 2^r, i + (k + 1) 2^r) -- so they tile the ring, once round
// or several times.  The common value is therefore the minimum of the whole ring: every min[i] is final.  The host still launches
// ceil(log2(crack_cap)) rounds, after which every window covers its ring whatever the flags say.
__global__ void __launch_bounds__(PG_THREADS) pg_min_round_kernel(const PgArgs a, int r) {
  long long count;
  if (!pg_live(a, count)) return;
  if (r > 0 && a.hdr[PG_H_FLAG_MIN + r - 1] == 0ull) return;
  const long long i = (long long)blockIdx.x * PG_THREADS + threadIdx.x;
  if (i == 0) a.hdr[PG_H_ROUNDS_MIN] = (u64)(r + 1);
  bool changed = false;
  if (i < count) {
    const int s = r & 1;
    const u64 mine = a.lead[s][i], far = a.lead[s][mine >> 32];
    const u32 m0 = (u32)mine, m1 = (u32)far;
    const u32 m = m1 < m0 ? m1 : m0;
    a.lead[s ^ 1][i] = (far & 0xffffffff00000000ull) | (u64)m;
    changed = m != m0;
  }
  pg_flag(a.hdr + PG_H_FLAG_MIN + r, changed);
}

// 5. the list of a ring: leader -> ... -> the crack whose successor is the leader
__global__ void __launch_bounds__(PG_THREADS) pg_cut_kernel(const PgArgs a) {
  long long count;
  if (!pg_live(a, count)) return;
  const long long i = (long long)blockIdx.x * PG_THREADS + threadIdx.x;
  if (i >= count) return;
  const u32 L = (u32)a.lead[(int)(a.hdr[PG_H_ROUNDS_MIN] & 1ull)][i];
  const u32 e = a.eid[i], s = a.succ[i];
  a.leader[i] = L;
  a.rank[0][i] = make_uint4(s == L ? PG_NIL : s, 1u, e >> 31, 0u);
  // x0 y1 - x1 y0 of the crack from (x0, y0) to (x1, y1): -y going east, x + 1 going south, y + 1 going west, -x going north
  const u32 id = e & ~PG_TURN;
  const long long p = id >> 2;
  const int d = (int)(id & 3u), y = (int)((u32)p / (u32)a.w), x = (int)p - y * a.w;
  const long long term = d == 0 ? -(long long)y : d == 1 ? (long long)x + 1 : d == 2 ? (long long)y + 1 : -(long long)x;
  if (term) atomicAdd(a.a2 + L, (u64)term);
}

// 6. round r: suffix sums by pointer jumping; a list of at most 2^r cracks is finished after r rounds
__global__ void __launch_bounds__(PG_THREADS) pg_rank_round_kernel(const PgArgs a, int r) {
  long long count;
  if (!pg_live(a, count)) return;
  if (r > 0 && a.hdr[PG_H_FLAG_RANK + r - 1] == 0ull) return;
  const long long i = (long long)blockIdx.x * PG_THREADS + threadIdx.x;
  if (i == 0) a.hdr[PG_H_ROUNDS_RANK] = (u64)(r + 1);
  bool changed = false;
  if (i < count) {
    const int s = r & 1;
    uint4 v = a.rank[s][i];
    if (v.x != PG_NIL) {
      const uint4 far = a.rank[s][v.x];
      v.x = far.x;
      v.y += far.y;
      v.z += far.z;
      changed = true;
    }
    a.rank[s ^ 1][i] = v;
  }
  pg_flag(a.hdr + PG_H_FLAG_RANK + r, changed);
}

// 7. every slot of the scan's input is written (the slots from `count` on are not read)
__global__ void __launch_bounds__(PG_THREADS) pg_ringkey_kernel(const PgArgs a) {
  long long count;
  if (!pg_live(a, count)) return;
  const long long i = (long long)blockIdx.x * PG_THREADS + threadIdx.x;
  if (i >= count) return;
  a.scan[i] = a.leader[i] == (u32)i ? (1ull << 32) | (u64)a.rank[(int)(a.hdr[PG_H_ROUNDS_RANK] & 1ull)][i].z : 0ull;
}

// 8. (id, label, byte, first vertex, vertices, cracks, A2) at the ring's number
__global__ void __launch_bounds__(PG_THREADS) pg_table_kernel(const PgArgs a) {
  long long count;
  if (!pg_live(a, count)) return;
  const long long i = (long long)blockIdx.x * PG_THREADS + threadIdx.x;
  if (i >= count || a.leader[i] != (u32)i) return;
  const u64 at = a.scan[i];
  const uint4 v = a.rank[(int)(a.hdr[PG_H_ROUNDS_RANK] & 1ull)][i];
  const long long ring = (long long)(at >> 32);
  if (ring >= a.ring_rows) return;                               // (a ring has at least 4 cracks: cannot happen)
  const long long id = a.eid[i] & ~PG_TURN, p = id >> 2;
  long long* row = a.table + ring * 7;
  row[0] = id;
  row[1] = a.label[p];
  row[2] = a.map[p];
  row[3] = (long long)(at & 0xffffffffull);
  row[4] = (long long)v.z;
  row[5] = (long long)v.y;
  row[6] = (long long)a.a2[i];
}

__global__ void pg_finish_kernel(const PgArgs a, u64* counters) {
  const u64 cracks = a.hdr[PG_H_CRACKS];
  const bool over = cracks > (u64)a.cap;
  const u64 total = over ? 0ull : a.hdr[PG_H_RINGTOTAL];
  a.hdr[PG_H_RINGS] = total >> 32;
  a.hdr[PG_H_VERTICES] = total & 0xffffffffull;
  a.hdr[PG_H_STATUS] = over ? 1ull : 0ull;
  a.hdr[PG_H_SHAPE] = ((u64)a.h << 32) | (u64)a.w;
  a.hdr[PG_H_CAP] = (u64)a.cap;
  counters[0] = cracks;
  counters[1] = total >> 32;
  counters[2] = total & 0xffffffffull;
  counters[3] = over ? 1ull : 0ull;
}

// ------------------------------------------------------------------------------------------------------------------ the outputs
// every thread decides alike from the header whether anything is written; thread 0 stores the status
__global__ void __launch_bounds__(PG_THREADS) pg_write_kernel(const PgArgs a, long long ring_cap, long long vertex_cap, long long* ring_table,
                                                              int* vertices, u32* status) {
  const long long i = (long long)blockIdx.x * PG_THREADS + threadIdx.x;
  const bool ok = a.hdr[PG_H_STATUS] == 0ull && a.hdr[PG_H_SHAPE] == (((u64)a.h << 32) | (u64)a.w) && a.hdr[PG_H_CAP] == (u64)a.cap &&
                  a.hdr[PG_H_CRACKS] <= (u64)a.cap && a.hdr[PG_H_RINGS] <= (u64)ring_cap && a.hdr[PG_H_VERTICES] <= (u64)vertex_cap &&
                  a.hdr[PG_H_RINGS] <= (u64)a.ring_rows;
  if (i == 0) *status = ok ? 0u : 1u;
  if (!ok || i >= (long long)a.hdr[PG_H_CRACKS]) return;
  const uint4* rank = a.rank[(int)(a.hdr[PG_H_ROUNDS_RANK] & 1ull)];
  const u32 L = a.leader[i], e = a.eid[i];
  const long long ring = (long long)(a.scan[L] >> 32);
  if (ring >= (long long)a.hdr[PG_H_RINGS]) return;              // (cannot happen in the scratch of a finished call)
  if (L == (u32)i) {
    const long long* row = a.table + ring * 7;
#pragma unroll
    for (int j = 0; j < 7; ++j) ring_table[ring * 7 + j] = row[j];
  }
  if (e & PG_TURN) {
    // the ordinal from the leader on: the ring's vertices less those from here to the end of the list, this one included
    const long long at = (long long)(a.scan[L] & 0xffffffffull) + (long long)rank[L].z - (long long)rank[i].z;
    if (at < 0 || at >= (long long)a.hdr[PG_H_VERTICES]) return; // (likewise)
    const u32 id = e & ~PG_TURN;
    const long long p = id >> 2;
    const int d = (int)(id & 3u), y = (int)((u32)p / (u32)a.w), x = (int)p - y * a.w;
    vertices[2 * at] = x + (d == 0 || d == 1 ? 1 : 0);
    vertices[2 * at + 1] = y + (d == 1 || d == 2 ? 1 : 0);
  }
}

bool pg_shape_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)h * (long long)w <= PG_MAX_PIXELS; }
bool pg_cap_ok(int h, int w, long long cap) { return cap >= 1 && cap <= 4LL * h * w; }
unsigned pg_grid(long long n) { return (unsigned)((n + PG_THREADS - 1) / PG_THREADS); }
int pg_log2_ceil(long long v) { int r = 0; while ((1LL << r) < v) ++r; return r; }

PgArgs pg_args(const unsigned char* map, const int* label, int h, int w, int connectivity, long long cap, void* scratch) {
  const PgLayout L = pg_layout((long long)h * w, cap);
  char* s = (char*)scratch;
  PgArgs a = {};
  a.map = map;
  a.label = label;
  a.hdr = (u64*)s;
  a.pixoff = (u32*)(s + L.pixoff);
  a.mask = (unsigned char*)(s + L.mask);
  a.eid = (u32*)(s + L.eid);
  a.succ = (u32*)(s + L.succ);
  a.leader = (u32*)(s + L.leader);
  a.rank[0] = (uint4*)(s + L.rank[0]);
  a.rank[1] = (uint4*)(s + L.rank[1]);
  a.lead[0] = (u64*)(s + L.rank[1]);
  a.lead[1] = a.lead[0] + cap;
  a.a2 = (u64*)(s + L.a2);
  a.scan = (u64*)(s + L.scan);
  a.table = (long long*)(s + L.table);
  a.h = h;
  a.w = w;
  a.conn8 = connectivity == 8 ? 1 : 0;
  a.cap = cap;
  a.ring_rows = L.ring_rows;
  return a;
}

}  // namespace

extern "C" {

int drs_polygon_count(const unsigned char* map, int h, int w, unsigned long long* counters, void* stream) {
  if (!map || !counters || !pg_shape_ok(h, w)) return DRS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  DRS_LAUNCH(pg_zero_kernel, dim3(1), dim3(PG_THREADS), 0, st, counters, 1);
  int rc = DRS_LAUNCH_CHECK();
  if (rc != DRS_OK) return rc;
  const unsigned need = pg_grid((long long)h * w);
  DRS_LAUNCH(pg_count_kernel, dim3(need < 4096u ? need : 4096u), dim3(PG_THREADS), 0, st, map, h, w, counters);
  return DRS_LAUNCH_CHECK();
}

size_t drs_polygon_scratch_bytes(int h, int w, int crack_cap) {
  if (!pg_shape_ok(h, w) || !pg_cap_ok(h, w, crack_cap)) return 0;
  return pg_layout((long long)h * w, crack_cap).bytes;
}

int drs_polygon_rings(const unsigned char* map, const int* label, int h, int w, int connectivity, int crack_cap, void* scratch,
                      unsigned long long* counters, void* stream) {
  if (!map || !label || !scratch || !counters || !pg_shape_ok(h, w) || (connectivity != 4 && connectivity != 8) || !pg_cap_ok(h, w, crack_cap))
    return DRS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)h * w;
  const PgLayout L = pg_layout(n, crack_cap);
  const PgArgs a = pg_args(map, label, h, w, connectivity, crack_cap, scratch);
  char* s = (char*)scratch;
  const unsigned pgrid = pg_grid(n), cgrid = pg_grid(crack_cap);
  int rc;
  DRS_LAUNCH(pg_zero_kernel, dim3(1), dim3(PG_THREADS), 0, st, a.hdr, (int)PG_H_WORDS);
  if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  DRS_LAUNCH(pg_mask_kernel, dim3(pgrid), dim3(PG_THREADS), 0, st, a);
  if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  if ((rc = pg_scan<u32>(a.pixoff, n, nullptr, (u32*)(s + L.psum1), (u32*)(s + L.psum2), a.hdr + PG_H_CRACKS, st)) != DRS_OK) return rc;
  DRS_LAUNCH(pg_build_kernel, dim3(pgrid), dim3(PG_THREADS), 0, st, a);
  if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  const int rounds = pg_log2_ceil(crack_cap);
  for (int r = 0; r < rounds; ++r) {
    DRS_LAUNCH(pg_min_round_kernel, dim3(cgrid), dim3(PG_THREADS), 0, st, a, r);
    if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  }
  DRS_LAUNCH(pg_cut_kernel, dim3(cgrid), dim3(PG_THREADS), 0, st, a);
  if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  for (int r = 0; r <= rounds; ++r) {
    DRS_LAUNCH(pg_rank_round_kernel, dim3(cgrid), dim3(PG_THREADS), 0, st, a, r);
    if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  }
  DRS_LAUNCH(pg_ringkey_kernel, dim3(cgrid), dim3(PG_THREADS), 0, st, a);
  if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  if ((rc = pg_scan<u64>(a.scan, crack_cap, a.hdr + PG_H_CRACKS, (u64*)(s + L.ssum1), (u64*)(s + L.ssum2), a.hdr + PG_H_RINGTOTAL, st)) != DRS_OK)
    return rc;
  DRS_LAUNCH(pg_table_kernel, dim3(cgrid), dim3(PG_THREADS), 0, st, a);
  if ((rc = DRS_LAUNCH_CHECK()) != DRS_OK) return rc;
  DRS_LAUNCH(pg_finish_kernel, dim3(1), dim3(1), 0, st, a, counters);
  return DRS_LAUNCH_CHECK();
}

int drs_polygon_write(const void* scratch, int h, int w, int crack_cap, int ring_cap, int vertex_cap, long long* ring_table,
                      int* vertices, unsigned int* status, void* stream) {
  if (!scratch || !ring_table || !vertices || !status || !pg_shape_ok(h, w) || !pg_cap_ok(h, w, crack_cap) || ring_cap < 0 || vertex_cap < 0)
    return DRS_ERR_ARG;
  const PgArgs a = pg_args(nullptr, nullptr, h, w, 4, crack_cap, const_cast<void*>(scratch));
  DRS_LAUNCH(pg_write_kernel, dim3(pg_grid(crack_cap)), dim3(PG_THREADS), 0, (hipStream_t)stream, a, ring_cap, vertex_cap, ring_table, vertices,
             status);
  return DRS_LAUNCH_CHECK();
}

}  // extern "C"
