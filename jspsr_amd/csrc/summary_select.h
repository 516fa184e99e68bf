// Device inlines the streaming selections of csrc/summary.hip (K12, K18) and csrc/strata.hip (K22) share: the ranks of a
// count, the order-preserving key, the wave sum and the ballot-aggregated histogram increment.  Moved here unchanged when
// K22 was added; both files are built with -ffp-contract=off.
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
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// One wave-instruction's worth of histogram increments (csrc/scores.hip: hist_add).  The top digit of a good
// prediction's errors falls into a handful of bins, and 64 lanes adding to one LDS address serialise: up to two rounds
// take the bin of the first pending lane, count its lanes with a ballot and let that lane add the count once.
// Every lane of the wave must arrive (wave-uniform trip counts at the call sites).
__device__ __forceinline__ void hist_add(unsigned* __restrict__ hist, bool match, unsigned bin) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const unsigned long long act = __ballot(match);
    if (act == 0ull) return;                                   // wave-uniform
    const int leader = __ffsll((long long)act) - 1;
    const unsigned b = (unsigned)__shfl((int)bin, leader, 64);
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

}  // namespace jspsr
