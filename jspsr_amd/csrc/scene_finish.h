// The parts that the entries after the model share (K8 tiles.hip, K12a summary.hip, K13 scene.hip, K14 scene_tta.hip, K15
// scene_tiles.hip): predictions -> metre rasters.
//   finish / finish_mean / merge: the prediction load and the metre conversion, one rounding per operation;
//   the epilogue that writes four consecutive pixels of a row;
//   the feather merge's ramp weight and its one accumulation step.  The three merge kernels keep their own loops: one
//   gather body over a cover policy measured 1.3 - 1.9 x slower on each of them (profiles/r32_finish_side_refactor.txt).
// Every translation unit that includes this is built with -ffp-contract=off (csrc/Makefile).
#pragma once
#include "common.h"

#include <cmath>

namespace jspsr {

// lo / span / log_span as the reference's Python forms them (doubles), rounded once to the tensors' fp32
struct ElevRange {
  float lo, span, log_span;
};
inline ElevRange elev_range(double elev_min, double elev_max) {
  return ElevRange{(float)elev_min, (float)(elev_max - elev_min), (float)log(elev_max - elev_min)};
}

__device__ __forceinline__ float load_pred(const void* p, size_t i, int bf16) {
  if (bf16) return __uint_as_float((unsigned int)static_cast<const unsigned short*>(p)[i] << 16);
  return static_cast<const float*>(p)[i];
}

// ToDEM.descale_data (data/data_utils.py:441-457): v (hi - lo) + lo, or exp(v log(hi - lo)) + lo.  Every operation rounded
// on its own, as the reference's element-wise tensor expressions are (no fused multiply-add: the scores are differences of
// de-scaled elevations of ~500 m, where a contraction moves the last bit and the median with it)
__device__ __forceinline__ float descale(float v, int elev_log, float lo, float span, float log_span) {
  return elev_log ? __fadd_rn(expf(__fmul_rn(v, log_span)), lo) : __fadd_rn(__fmul_rn(v, span), lo);
}

// A prediction in metres: clamp (a NaN stays a NaN, as torch.clamp leaves it), descale, + base -- the bits of
// summary.compose_scene
__device__ __forceinline__ float to_metres(float t, int elev_log, float lo, float span, float log_span, float base) {
  t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
  return __fadd_rn(descale(t, elev_log, lo, span, log_span), base);
}

// Four consecutive pixels of an output row, n of them inside it: one 16-byte store where the caller found o aligned
__device__ __forceinline__ void store_quad(float* o, const float (&v)[4], int n, bool vec) {
  if (vec) {
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int q = 0; q < n; ++q) o[q] = v[q];
  }
}

// weight of position j (0 .. w_l_c-1) of a tile at cover position pos (0 .. n_x-1): 1 inside, the linear ramp over the
// p = w_l_c - s pixels it shares with a neighbour (utils.py:802-895: linspace(1, 0, p + 2) without its ends); where the
// rising and the falling ramp meet (2 p > w_l_c) the falling one wins
__device__ __forceinline__ float ramp_weight(const float* __restrict__ ramp, int p, int w_l_c, int n_x, int pos, int j) {
  float w = 1.f;
  if (pos > 0 && j < p) w = ramp[p - 1 - j];
  if (pos < n_x - 1 && j >= w_l_c - p) w = ramp[j - (w_l_c - p)];
  return w;
}

// acc + (m * wx) * wy, every product and the sum rounded on its own: merge_dem's tile * wx * wy added to the mosaic tile by
// tile.  (hipcc contracts a * b + c into a fused multiply-add by default, __fmul_rn / __fadd_rn included: hence the
// -ffp-contract=off above)
__device__ __forceinline__ float feather_add(float acc, float m, float wx, float wy) {
  return __fadd_rn(acc, __fmul_rn(__fmul_rn(m, wx), wy));
}

}  // namespace jspsr
