// K13 -- whole-scene inference, the step after the forward (upscale_dem, utils/utils.py:1556-1654; the step before it,
// jspsr_scene_prepare, is in scene_prepare.hip):
//   jspsr_scene_finish    remove_padding (utils.py:1523-1531) and, for metres, clip -> descale_data -> + base
//                         (evaluation/evaluate_utils.py:242-271), ONE launch
// HBM streaming, 4 B in, 4 B out.  No LDS: a thread makes four consecutive pixels of a row of the scene's window, so a wave
// writes 1 KiB runs (16-byte stores when W % 4 == 0 and the output is 16-byte aligned).
#include "scene_finish.h"

namespace {

using namespace jspsr;

// out[b][y][x] = pred[b][top + y][left + x], in metres (to_metres) or as it is
__global__ __launch_bounds__(256) void scene_finish_kernel(const void* __restrict__ pred, float* __restrict__ out,
                                                          const int* __restrict__ samples, int bf16, int B, int Hp, int Wp,
                                                          int top, int left, int H, int W, int metres, int elev_log, ElevRange e,
                                                          int vec) {
  const int Wq = (W + 3) >> 2;
  const long long total = (long long)B * H * Wq;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % Wq) * 4;
    const long long r = i / Wq;
    const int y = (int)(r % H), b = (int)(r / H);
    const int n = min(4, W - x);
    const float base = __int_as_float(samples[2 * b + 1]);
    const size_t s = ((size_t)b * Hp + top + y) * Wp + left + x;
    float v[4];
    for (int q = 0; q < 4; ++q) {
      const float t = load_pred(pred, s + min(q, n - 1), bf16);
      v[q] = metres ? to_metres(t, elev_log, e.lo, e.span, e.log_span, base) : t;
    }
    store_quad(out + ((size_t)b * H + y) * W + x, v, n, vec);
  }
}

}  // namespace

extern "C" int jspsr_scene_finish(int dtype, const void* pred, float* out, const int* samples, int B, int Hp, int Wp, int top,
                                  int left, int H, int W, int metres, int elev_log, double elev_min, double elev_max,
                                  jspsr_stream_t stream) {
  if (!pred || !out || !samples || B <= 0 || Hp <= 0 || Wp <= 0 || H <= 0 || W <= 0 || !(elev_max > elev_min) ||
      (dtype != JSPSR_F32 && dtype != JSPSR_BF16))
    return jspsr::fail(JSPSR_EINVAL, "scene_finish: bad arguments");
  if (top < 0 || left < 0 || (long long)top + H > Hp || (long long)left + W > Wp)
    return jspsr::fail(JSPSR_EINVAL, "scene_finish: the window (%d, %d) + %d x %d leaves the %d x %d frame", top, left, H, W, Hp, Wp);
  const int bf16 = dtype == JSPSR_BF16;
  if (!jspsr::aligned4(out) || (reinterpret_cast<uintptr_t>(pred) & (bf16 ? 1u : 3u)))
    return jspsr::fail(JSPSR_EALIGN, "scene_finish: pointers not aligned to their element size");
  const long long items = (long long)B * H * ((W + 3) / 4);
  hipLaunchKernelGGL(scene_finish_kernel, dim3(blocks_for(items)), dim3(256), 0, static_cast<hipStream_t>(stream), pred, out, samples,
                     bf16, B, Hp, Wp, top, left, H, W, metres ? 1 : 0, elev_log ? 1 : 0, elev_range(elev_min, elev_max),
                     (W & 3) == 0 && jspsr::aligned16(out));
  return jspsr::check_launch("scene_finish");
}
