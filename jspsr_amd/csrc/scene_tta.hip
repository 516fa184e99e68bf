// K14 -- whole-scene self-ensemble (the "+" of EDSR+), the step after the forwards (the step before them,
// jspsr_scene_prepare_d4, is in scene_prepare.hip):
//   jspsr_scene_finish_mean  the inverse transform of up to eight predictions, their fp32 mean in the order given, and K13's
//                            metre conversion, ONE launch
//
// finish_mean: one workgroup makes one 32 x 32 tile of one scene's result.  An even variant's four pre-images are consecutive
// in a row of its prediction (forwards or backwards) and are read from memory directly, 128-byte runs per eight lanes.  An odd
// variant's lie in a column: its 32 x 32 tile of the prediction is staged with row-contiguous loads in lds[slot][32][33]
// (16.9 KiB: of eight distinct elements four are quarter turns, and the entry point refuses duplicates) and read transposed --
// pitch 33: lane (oy, ox) reads bank (ox + p + oy) mod 32 up to reflection, and within 32 lanes ox is a multiple of 4 and oy
// spans 4 values: conflict-free.
#include "scene_finish.h"
#include "scene_prepare.h"   // kTile, d4_image

#include <climits>

namespace {

using namespace jspsr;

constexpr int kPredPitch = kTile + 1;                       // floats
constexpr int kVariants = JSPSR_TTA_MAX_VARIANTS;
constexpr int kOddVariants = 4;                             // the quarter turns among eight distinct elements

struct Variant {
  const void* pred;           // [B][1][Hp][Wp]
  int bf16, code, Hp, Wp, top, left;
};

struct MeanArgs {
  Variant v[kVariants];
  float* out;                 // [B][H][W]
  const int* samples;         // [B][2] {scene, base (fp32 bits)}
  int K, B, H, W, metres, elev_log, vec;
  ElevRange e;
  float count;
};

// out[b][y][x] = post((((y'_0 + y'_1) + y'_2) + ...) / K), y'_k[y][x] = pred_k[b][top_k + i][left_k + j] with (i, j) the
// image of (y, x) under element k; post = to_metres, or nothing
__global__ __launch_bounds__(256) void scene_finish_mean_kernel(MeanArgs a, int tiles_x) {
  __shared__ float lds[kOddVariants][kTile * kPredPitch];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int y0 = (blockIdx.x / tiles_x) * kTile, x0 = (blockIdx.x % tiles_x) * kTile;
  const int th = min(kTile, a.H - y0), tw = min(kTile, a.W - x0);
  for (int k = 0, slot = 0; k < a.K && slot < kOddVariants; ++k) {
    const Variant& v = a.v[k];
    if (!(v.code & 4)) continue;
    // the tile's image in an odd variant: tw rows (from x) by th columns (from y); two opposite corners span it
    int ia, ja, ib, jb;
    d4_image(v.code, a.H, a.W, y0, x0, ia, ja);
    d4_image(v.code, a.H, a.W, y0 + th - 1, x0 + tw - 1, ib, jb);
    const int i0 = min(ia, ib), j0 = min(ja, jb);
    for (int idx = tid; idx < tw * th; idx += 256) {
      const int r = idx / th, c = idx - r * th;
      lds[slot][r * kPredPitch + c] = load_pred(v.pred, ((size_t)b * v.Hp + v.top + i0 + r) * v.Wp + v.left + j0 + c, v.bf16);
    }
    ++slot;
  }
  __syncthreads();

  const int oy = tid >> 3, ox = (tid & 7) * 4;
  if (oy >= th || ox >= tw) return;
  const int n = min(4, tw - ox);
  const int y = y0 + oy;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int slot = -1;
  for (int k = 0; k < a.K; ++k) {
    const Variant& v = a.v[k];
    int i0 = 0, j0 = 0;
    if (v.code & 4) {
      slot = min(slot + 1, kOddVariants - 1);
      int ia, ja, ib, jb;
      d4_image(v.code, a.H, a.W, y0, x0, ia, ja);
      d4_image(v.code, a.H, a.W, y0 + th - 1, x0 + tw - 1, ib, jb);
      i0 = min(ia, ib); j0 = min(ja, jb);
    }
    for (int q = 0; q < 4; ++q) {
      int i, j;
      d4_image(v.code, a.H, a.W, y, x0 + ox + min(q, n - 1), i, j);
      const float t = (v.code & 4) ? lds[slot][(i - i0) * kPredPitch + (j - j0)]
                                   : load_pred(v.pred, ((size_t)b * v.Hp + v.top + i) * v.Wp + v.left + j, v.bf16);
      acc[q] = k == 0 ? t : __fadd_rn(acc[q], t);
    }
  }
  const float base = __int_as_float(a.samples[2 * b + 1]);
  float r[4];
  for (int q = 0; q < 4; ++q) {
    const float t = __fdiv_rn(acc[q], a.count);                       // K = 1: x / 1.0f is x
    r[q] = a.metres ? to_metres(t, a.elev_log, a.e.lo, a.e.span, a.e.log_span, base) : t;
  }
  store_quad(a.out + ((size_t)b * a.H + y) * a.W + x0 + ox, r, n, a.vec);
}

// The element a code denotes, as the code with flip_ud clear: flipud = fliplr after a half turn
int canonical(int code) { return (code & 1) ? ((((code >> 2) + 2) & 3) << 2) | ((code & 2) ^ 2) : code; }

}  // namespace

extern "C" int jspsr_scene_finish_mean(const jspsr_tta_variant* variants, int K, float* out, const int* samples, int B, int H,
                                       int W, int metres, int elev_log, double elev_min, double elev_max, jspsr_stream_t stream) {
  if (!variants || !out || !samples || B <= 0 || B > 65535 || H <= 0 || W <= 0 || !(elev_max > elev_min))
    return jspsr::fail(JSPSR_EINVAL, "scene_finish_mean: bad arguments");
  if (K < 1 || K > kVariants) return jspsr::fail(JSPSR_EINVAL, "scene_finish_mean: %d variants, 1..%d are taken", K, kVariants);
  if (!jspsr::aligned4(out)) return jspsr::fail(JSPSR_EALIGN, "scene_finish_mean: output not 4-byte aligned");
  MeanArgs a{};
  for (int k = 0; k < K; ++k) {
    const jspsr_tta_variant& v = variants[k];
    if (!v.pred || (v.dtype != JSPSR_F32 && v.dtype != JSPSR_BF16) || v.code < 0 || v.code > 15 || v.Hp <= 0 || v.Wp <= 0)
      return jspsr::fail(JSPSR_EINVAL, "scene_finish_mean: variant %d: bad arguments", k);
    for (int m = 0; m < k; ++m)
      if (canonical(variants[m].code) == canonical(v.code))
        return jspsr::fail(JSPSR_EINVAL, "scene_finish_mean: variants %d and %d (codes %d, %d) are the same element", m, k,
                           variants[m].code, v.code);
    const int odd = (v.code >> 2) & 1, h = odd ? W : H, w = odd ? H : W;
    if (v.h != h || v.w != w)
      return jspsr::fail(JSPSR_EINVAL, "scene_finish_mean: variant %d (code %d): a %d x %d window, the %d x %d scene transforms to %d x %d",
                         k, v.code, v.h, v.w, H, W, h, w);
    if (v.top < 0 || v.left < 0 || (long long)v.top + h > v.Hp || (long long)v.left + w > v.Wp)
      return jspsr::fail(JSPSR_EINVAL, "scene_finish_mean: variant %d: the window (%d, %d) + %d x %d leaves the %d x %d frame", k,
                         v.top, v.left, h, w, v.Hp, v.Wp);
    const int bf16 = v.dtype == JSPSR_BF16;
    if (reinterpret_cast<uintptr_t>(v.pred) & (bf16 ? 1u : 3u))
      return jspsr::fail(JSPSR_EALIGN, "scene_finish_mean: variant %d: predictions not aligned to their element size", k);
    a.v[k] = Variant{v.pred, bf16, v.code, v.Hp, v.Wp, v.top, v.left};
  }
  a.out = out;
  a.samples = samples;
  a.K = K;
  a.B = B;
  a.H = H;
  a.W = W;
  a.metres = metres ? 1 : 0;
  a.elev_log = elev_log ? 1 : 0;
  a.vec = (W & 3) == 0 && jspsr::aligned16(out);
  a.e = elev_range(elev_min, elev_max);
  a.count = (float)K;
  const long long tiles_x = (W + kTile - 1) / kTile, tiles = tiles_x * ((H + kTile - 1) / kTile);
  if (tiles > INT_MAX) return jspsr::fail(JSPSR_EINVAL, "scene_finish_mean: a %d x %d scene has too many tiles", H, W);
  hipLaunchKernelGGL(scene_finish_mean_kernel, dim3((unsigned)tiles, B), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     (int)tiles_x);
  return jspsr::check_launch("scene_finish_mean");
}
