// The folds of the loss family (csrc/train_step.hip: L1 + L2 + Sobel; csrc/loss_terms.hip: the menu): three float sums of a
// workgroup, with NC integer counts beside them, into per-workgroup partials, and the fixed-order folds of those partials
// by one wave.  Every order is fixed, so every run gives the same bits.
#pragma once
#include "common.h"

namespace jspsr {

// T threads: partial[3 * block + q] = the workgroup's sum of v[q], pcnt[NC * block + q] = its sum of c[q].  Wave sums by
// xor shuffles, then waves 0 .. T/64 - 1 in order.  red: 3 * T/64 floats of LDS, redc: NC * T/64 words (NC = 0: unused).
template <int T, int NC>
__device__ __forceinline__ void block_fold3(float (&v)[3], unsigned int* c, float* red, unsigned int* redc,
                                            float* __restrict__ partial, unsigned int* __restrict__ pcnt) {
  constexpr int NW = T / 64;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
    if ((threadIdx.x & 63) == 0) red[q * NW + (threadIdx.x >> 6)] = v[q];
  }
#pragma unroll
  for (int q = 0; q < NC; ++q) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c[q] += __shfl_xor(c[q], d, 64);
    if ((threadIdx.x & 63) == 0) redc[q * NW + (threadIdx.x >> 6)] = c[q];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float t = 0.f;
    for (int w = 0; w < NW; ++w) t += red[threadIdx.x * NW + w];
    partial[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
  } else if (threadIdx.x < 3 + NC) {
    unsigned int t = 0;
    for (int w = 0; w < NW; ++w) t += redc[(threadIdx.x - 3) * NW + w];
    pcnt[(size_t)blockIdx.x * NC + threadIdx.x - 3] = t;
  }
}

// Double fold of `rows` partials of column q (row stride `cols`) by one wave; the sum lands in every lane.  p NULL: 0.
__device__ __forceinline__ double wave_fold(const float* __restrict__ p, int rows, int cols, int q) {
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  if (p)
    for (int r = lane; r < rows; r += 64) s += (double)p[(size_t)r * cols + q];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

// The same walk over per-workgroup counts, in integers.
__device__ __forceinline__ long long wave_count(const unsigned int* __restrict__ p, int rows, int cols, int q) {
  const int lane = threadIdx.x & 63;
  long long s = 0;
  if (p)
    for (int r = lane; r < rows; r += 64) s += (long long)p[(size_t)r * cols + q];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  return s;
}

}  // namespace jspsr
