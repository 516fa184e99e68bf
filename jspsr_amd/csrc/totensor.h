// ToTensor's per-kind arithmetic (data/data_utils.py:217-312), shared by K9 (batch.hip) and K13-K16 (scene_prepare.hip) so that all
// give the same bits.  Every operation is rounded on its own: the translation units that include this are built with
// -ffp-contract=off (csrc/Makefile).
//
// `A` is the kernel's argument block; it carries
//   int flags (JSPSR_BATCH_*), mask_div;  float lo = fp32(elev_min), span = fp32(elev_max - elev_min);
//   double log_span = log(elev_max - elev_min), as the reference's np.log of a Python number.
#pragma once
#include "common.h"

#include <cmath>

namespace jspsr {

enum Kind { LR_DEM = 0, HR_DEM = 1, IMAGE = 2, MASK = 3, CANOPY = 4, COORD = 5 };
constexpr int kKinds = 6;
constexpr int kMaxC = 16;                                   // channels per kind

template <class A>
__device__ __forceinline__ float scale_dem(float z, float base, int is_label, const A& a) {
  float v = z;
  if (base != 0.f) v = __fsub_rn(v, base);                            // data - base_elev (fp32)
  v = __fsub_rn(v, a.lo);                                             // data - elev_min (fp32)
  const bool to11 = (a.flags & (is_label ? JSPSR_BATCH_LABEL_11 : JSPSR_BATCH_IMAGE_11)) != 0;
  if (a.flags & JSPSR_BATCH_LOG) {
    // np.log(fp32) / np.log(<Python number>) is fp32 / float64 -> float64 under NumPy 2, and so are + 1e-8 and * 2 - 1
    double o = __dadd_rn(__ddiv_rn((double)logf(v), a.log_span), 1e-8);
    if (to11) o = __dsub_rn(__dmul_rn(o, 2.0), 1.0);
    return (float)o;
  }
  float o = __fdiv_rn(v, a.span);                                     // (data - min) / (max - min), fp32
  if (to11) o = __fsub_rn(__fmul_rn(o, 2.f), 1.f);
  return o;
}

// p: the channel's value in the scene store (fp32 for the DEMs, one byte otherwise; unused for COORD); (Y, X) the source
// pixel in its H x W scene (COORD only)
template <class A>
__device__ __forceinline__ float transform(int kind, int c, const unsigned char* p, float base, int Y, int X, long long H,
                                           long long W, const A& a) {
  switch (kind) {
    case LR_DEM: return scale_dem(*reinterpret_cast<const float*>(p), base, 0, a);
    case HR_DEM: return scale_dem(*reinterpret_cast<const float*>(p), base, 1, a);
    case IMAGE: {
      float o = __fdiv_rn((float)*p, 255.f);                          // to_tensor: uint8 -> float, div(255)
      if (a.flags & JSPSR_BATCH_IMAGE_11) o = __fsub_rn(__fmul_rn(2.f, o), 1.f);
      else if (a.flags & JSPSR_BATCH_IMAGE_255) o = __fdiv_rn(o, 255.f);
      return o;
    }
    case MASK:
      if (a.flags & JSPSR_BATCH_SCALE_MASK) return __fdiv_rn(__fmul_rn((float)*p, (float)(c + 1)), (float)a.mask_div);
      return (float)*p;
    case CANOPY: return __fdiv_rn((float)*p, 68.f);
    default:                                                          // local coordinates over the whole scene
      return c == 0 ? __fdiv_rn((float)Y, (float)(H - 1)) : __fdiv_rn((float)X, (float)(W - 1));
  }
}

}  // namespace jspsr
