// Device inlines every selection on order-preserving keys shares: csrc/metrics.hip (K7), csrc/scores.hip (K10, K20),
// csrc/summary.hip (K12, K18), csrc/errdist.hip (K21) and csrc/strata.hip (K22).  The key and its inverse, the select
// transform, the wave sum, the ballot-aggregated histogram increment, the table bisection; for the pooled family the ranks
// of a count, the row state, the rank scan and the replica rule.  The first group is integer code and plain adds, the same
// bits under any contraction flag; segment_ranks_of and rank_scan round step by step and are used only by files built with
// -ffp-contract=off (summary.hip, strata.hip).
#pragma once
#include "common.h"

#include <cmath>

namespace jspsr {

// The ranks and the weight every order statistic of n >= 1 elements is read at (jspsr_amd/summary.py: segment_ranks):
// median (n - 1) / 2 and n / 2; v = 0.95 (n - 1) in double, l = floor(v), LE95 l and min(l + 1, n - 1), g = v - l.  No
// contraction (-ffp-contract=off): v is rounded before floor(v) is taken from it.
struct Ranks {
  long long m0, m1, l0, l1;
  double g;
};
__host__ __device__ inline Ranks segment_ranks_of(long long n) {
  Ranks r;
  const double v = 0.95 * (double)(n - 1);
  const double fl = floor(v);
  r.m0 = (n - 1) / 2;
  r.m1 = n / 2;
  r.l0 = (long long)fl;
  r.l1 = r.l0 + 1 < n - 1 ? r.l0 + 1 : n - 1;
  r.g = v - fl;
  return r;
}

__device__ __forceinline__ unsigned order_key(float f) {      // float -> unsigned key with the same ordering (NaNs last)
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// what a per-tile select orders (K7, K10, K20).  mode 0: x; 1: |x - center|; 2: |x|
__device__ __forceinline__ float sel_transform(float x, int mode, float center) {
  return mode == 0 ? x : (mode == 1 ? fabsf(x - center) : fabsf(x));
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// One wave-instruction's worth of histogram increments.  The top digit of a good prediction's errors falls into a handful
// of bins, and 64 lanes adding to one LDS address serialise: up to ROUNDS times take the bin of the first pending lane,
// count its lanes with a ballot and let that lane add the count once; what is left adds singly.  Every lane of the wave
// must arrive (wave-uniform trip counts at the call sites).  READLANE: the leader is wave-uniform, so its bin can come by
// v_readlane instead of the LDS permute of __shfl.  K21's single call per element is built that way; behind the four to
// sixteen calls per element of the K10 / K12 / K18 / K22 kernels the compiler then keeps a branch around every round
// where it predicates the __shfl form (summary_select_kernel: 70 exec branches against 6, 4 - 9 % slower on an MI355X,
// profiles/r26_pooled_family_refactor.txt), so those keep the permute.
template <int ROUNDS = 2, bool READLANE = false>
__device__ __forceinline__ void hist_add(unsigned* __restrict__ hist, bool match, unsigned bin) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < ROUNDS; ++it) {
    const unsigned long long act = __ballot(match);
    if (act == 0ull) return;                                   // wave-uniform
    const int leader = __ffsll((long long)act) - 1;
    const unsigned b = READLANE ? (unsigned)__builtin_amdgcn_readlane((int)bin, leader) : (unsigned)__shfl((int)bin, leader, 64);
    const bool mine = match && bin == b;
    const unsigned long long m = __ballot(mine);
    if (lane == leader) atomicAdd(&hist[b], (unsigned)__popcll(m));
    match = match && !mine;
  }
  if (match) atomicAdd(&hist[bin], 1u);
}

// last row whose word `col` is <= v (rows ascending in that word; row 0 if none is)
__device__ __forceinline__ int find_row(const long long* __restrict__ tab, int rows, int words, int col, long long v) {
  int lo = 0, hi = rows - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[(size_t)mid * words + col] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- the pooled family (K12, K18, K22): one row of eleven scores per (candidate, segment or class) --------------------
constexpr int SCAN_MT = 256;                  // threads of a scan workgroup: a wave per state
constexpr int NSTATE = 6;                     // ranks: median lo, hi | LE95 lo, hi | MAD lo, hi
constexpr int NOUT = 11;                      // RMSE, Median, NMAD, LE95, PSNR, med lo, hi, mad lo, hi, le lo, hi

struct RowState {            // one per row, in device memory; 64 bytes
  unsigned prefix[NSTATE];   // key bits fixed so far (high bits)
  unsigned k[NSTATE];        // rank still to find inside the current prefix class (0-based)
  float center;              // the median, for |e - median|
  unsigned has_nan;          // bit 0: the fp64 sum is NaN, a NaN among the errors; bit 1: the row has no element (never set by K12)
  unsigned g[2];             // the bits of the LE95 weight where the count is data on the device (K12 reads the segment table's)
};
static_assert(sizeof(RowState) == 64, "RowState layout");

// Replicas of a row's histograms.  Every workgroup of a row ends in global adds to the row's 256 counters per state; to one
// address they serialise, and a 4096 x 4096 segment has 2048 workgroups.  Chunk c adds to replica c % reps, the scan sums
// the replicas: integer counts, so the result does not depend on reps.  A power of two, at most 16, one per 64 chunks of
// the call, and at most 64 MiB of counters (K22's at most 8 x 32 rows never reach that: 48 MiB at 16 replicas).
inline int hist_replicas(size_t rows, long long chunks) {
  int r = 1;
  while (r < 16 && (long long)r * 64 < chunks && rows * (size_t)(2 * r) * NSTATE * 256 * sizeof(unsigned) <= ((size_t)64 << 20)) r *= 2;
  return r;
}

// The part of a scan every row shares, a workgroup of SCAN_MT threads per row, a wave per state: find the bin holding the
// state's rank, fix its byte, reduce the rank; clear the row's histograms; after byte 0 the keys are complete and the
// scores are written; the state goes back to device memory.  cur: the row's state in LDS, complete behind a barrier (the
// caller's init block formed it from its own count and sum, or loaded it).  hrow: the row's `reps` replicas, back to back.
// g_bits: the fp64 bits of the LE95 weight.
__device__ __forceinline__ void rank_scan(RowState& cur, const void* g_bits, unsigned* __restrict__ hrow, int reps, int group, int pass,
                                          float* __restrict__ o, RowState* __restrict__ st_row) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = (group ? 4 : 0) + wave, ql = q & ~1;
  const bool active = group ? wave < 2 : true;
  const int shift = pass * 8;
  const unsigned himask = pass == 3 ? 0u : (0xffffffffu << (shift + 8));
  unsigned new_prefix = 0u, new_k = 0u;
  bool found = false;
  if (active) {
    const unsigned prefix = cur.prefix[q], k = cur.k[q];
    const bool same = ((prefix ^ cur.prefix[ql]) & himask) == 0u;       // counted once, under the pair's lower state
    const unsigned* h = hrow + (same ? ql : q) * 256 + 4 * lane;         // lane l owns bins 4l .. 4l+3
    unsigned c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
    for (int r = 0; r < reps; ++r) {
      const uint4 v = *reinterpret_cast<const uint4*>(h + (size_t)r * NSTATE * 256);
      c0 += v.x; c1 += v.y; c2 += v.z; c3 += v.w;
    }
    const unsigned own = c0 + c1 + c2 + c3;
    unsigned incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl += up;
    }
    const unsigned excl = incl - own;
    if (k >= excl && k < incl) {                                 // exactly one lane: the counts sum to more than k (none: an empty row)
      unsigned run = excl;
      int b = 0;
      if (k >= run + c0) { run += c0; b = 1;
        if (k >= run + c1) { run += c1; b = 2;
          if (k >= run + c2) { run += c2; b = 3; } } }
      new_k = k - run;
      new_prefix = prefix | ((unsigned)(4 * lane + b) << shift);
      found = true;
    }
  }
  __syncthreads();                                               // every wave has read the states and its histogram
  if (found) { cur.prefix[q] = new_prefix; cur.k[q] = new_k; }
  {                                                              // clear what this group's passes count into: states 0..3 or 4, 5
    const int first = group ? 4 : 0, quads = (group ? 2 : 4) * 64; // uint4 per replica
    for (int i = tid; i < reps * quads; i += SCAN_MT)
      reinterpret_cast<uint4*>(hrow + ((size_t)(i / quads) * NSTATE + first) * 256)[i % quads] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  if (pass == 0 && tid == 0) {
    const float nanv = __builtin_nanf("");
    const bool bad = cur.has_nan != 0u, empty = (cur.has_nan & 2u) != 0u;   // a NaN row keeps its brackets, an empty one has none
    if (!group) {
      const float m0 = key_value(cur.prefix[0]), m1 = key_value(cur.prefix[1]);
      const float l0 = key_value(cur.prefix[2]), l1 = key_value(cur.prefix[3]);
      const float med = __fmul_rn(__fadd_rn(m0, m1), 0.5f);      // np.median of a float32 array: mean of the two middle elements
      double g;
      __builtin_memcpy(&g, g_bits, 8);
      const float le = (float)((double)l0 + ((double)l1 - (double)l0) * g);
      cur.center = med;
      o[1] = bad ? nanv : med;
      o[3] = bad ? nanv : le;
      o[5] = empty ? nanv : m0; o[6] = empty ? nanv : m1; o[9] = empty ? nanv : l0; o[10] = empty ? nanv : l1;
      if (bad) { o[0] = nanv; o[4] = nanv; }
    } else {
      const float d0 = key_value(cur.prefix[4]), d1 = key_value(cur.prefix[5]);
      const float mad = __fmul_rn(__fadd_rn(d0, d1), 0.5f);
      o[2] = bad ? nanv : (float)(1.4826 * (double)mad);
      o[7] = empty ? nanv : d0; o[8] = empty ? nanv : d1;
    }
  }
  __syncthreads();
  if (tid < (int)(sizeof(RowState) / 4)) reinterpret_cast<unsigned*>(st_row)[tid] = reinterpret_cast<const unsigned*>(&cur)[tid];
}

}  // namespace jspsr
