// K15 -- tiled whole-scene inference, the step after the forwards (jspsr_amd/infer.py: plan_cover, predict_scenes; the step
// before them, jspsr_scene_prepare_windows, is in scene_prepare.hip):
//   jspsr_scene_merge_windows     the predictions of the cover of S equally shaped scenes -> S metre rasters: per tile
//                                 clamp -> descale_data -> + base, then the feather merge with the cover's ramp weights
//                                 (TileCrop / merge_dem's protocol, utils/utils.py:802-967, for any cover), ONE launch
// HBM streaming with jspsr_scene_finish's access pattern (csrc/scene.hip): no LDS, a thread makes four consecutive pixels of
// a row, a wave writes 1 KiB runs (16-byte stores when the row length is a multiple of 4 and the output is 16-byte aligned).
// It reads 4 B (2 B for bf16) per covered tile pixel -- one tile inside, two in a seam, four at a seam crossing -- and
// writes 4 B.  The merge is a gather: every output pixel sums its own tiles in row-major order, no atomics, the same bits on
// every run.
//
// All offsets into the tile buffer and the output are 64-bit: the cover of a 37 000 x 37 000 scene passes 2^31 bytes.
#include "scene_finish.h"

namespace {

using namespace jspsr;

struct MergeArgs {
  const void* tiles;          // [S][n_y * n_x][kh][kw], fp32 or bf16
  const float* wy;            // [n_y][kh] row weights of every tile row of the cover
  const float* wx;            // [n_x][kw]
  const int* lo_y;            // [H] lowest tile row with a non-zero weight at y
  const int* lo_x;            // [W]
  const int* oy;              // [n_y] tile origins
  const int* ox;              // [n_x]
  const int* samples;         // [S][2] {scene, base (fp32 bits)}
  float* out;                 // [S][H][W]
  int bf16, S, n_y, n_x, kh, kw, H, W, metres, elev_log, vec;
  ElevRange e;
};

// out[s][y][x] = sum over the (at most 2 x 2) tiles with non-zero weights there, row-major, of (m * wx) * wy; m the tile
// value in metres (to_metres) or as it is.  The sum is scenes_assemble_kernel's
// (csrc/summary.hip): acc starts at 0 and takes feather_add.
__global__ __launch_bounds__(256) void scene_merge_windows_kernel(MergeArgs a) {
  const int Wq = (a.W + 3) >> 2;
  const long long total = (long long)a.S * a.H * Wq;
  const size_t tile = (size_t)a.kh * a.kw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x0 = (int)(i % Wq) * 4;
    const long long r = i / Wq;
    const int y = (int)(r % a.H), s = (int)(r / a.H);
    const int n = min(4, a.W - x0);
    const float base = __int_as_float(a.samples[2 * s + 1]);
    const int ty0 = a.lo_y[y];
    int jy[2];
    float wy[2];
    for (int u = 0; u < 2; ++u) {
      const int ty = ty0 + u;
      jy[u] = -1;
      wy[u] = 0.f;
      if (ty0 >= 0 && ty < a.n_y) {
        const int j = y - a.oy[ty];
        if (j >= 0 && j < a.kh) { jy[u] = j; wy[u] = a.wy[(size_t)ty * a.kh + j]; }
      }
    }
    float v[4];
    for (int q = 0; q < 4; ++q) {
      const int x = x0 + min(q, n - 1);
      const int tx0 = a.lo_x[x];
      int jx[2];
      float wx[2];
      for (int u = 0; u < 2; ++u) {
        const int tx = tx0 + u;
        jx[u] = -1;
        wx[u] = 0.f;
        if (tx0 >= 0 && tx < a.n_x) {
          const int j = x - a.ox[tx];
          if (j >= 0 && j < a.kw) { jx[u] = j; wx[u] = a.wx[(size_t)tx * a.kw + j]; }
        }
      }
      float acc = 0.f;
      for (int u = 0; u < 2; ++u) {
        if (jy[u] < 0 || wy[u] == 0.f) continue;
        for (int w = 0; w < 2; ++w) {
          if (jx[w] < 0 || wx[w] == 0.f) continue;                     // a tile of weight zero is not read
          const size_t t = ((size_t)s * a.n_y + (ty0 + u)) * a.n_x + (tx0 + w);
          float m = load_pred(a.tiles, t * tile + (size_t)jy[u] * a.kw + jx[w], a.bf16);
          if (a.metres) m = to_metres(m, a.elev_log, a.e.lo, a.e.span, a.e.log_span, base);
          acc = feather_add(acc, m, wx[w], wy[u]);
        }
      }
      v[q] = acc;
    }
    store_quad(a.out + ((size_t)s * a.H + y) * a.W + x0, v, n, a.vec);
  }
}

}  // namespace

extern "C" int jspsr_scene_merge_windows(int dtype, const void* tiles, const float* wy, const float* wx, const int* lo_y,
                                         const int* lo_x, const int* oy, const int* ox, const int* samples, float* out, int S,
                                         int n_y, int n_x, int kh, int kw, int H, int W, int metres, int elev_log,
                                         double elev_min, double elev_max, jspsr_stream_t stream) {
  if (!tiles || !wy || !wx || !lo_y || !lo_x || !oy || !ox || !samples || !out || S <= 0 || n_y <= 0 || n_x <= 0 || kh <= 0 ||
      kw <= 0 || H <= 0 || W <= 0 || !(elev_max > elev_min) || (dtype != JSPSR_F32 && dtype != JSPSR_BF16))
    return jspsr::fail(JSPSR_EINVAL, "scene_merge_windows: bad arguments");
  if (kh > H || kw > W || (long long)n_y * kh < H || (long long)n_x * kw < W)
    return jspsr::fail(JSPSR_EINVAL, "scene_merge_windows: %d x %d tiles of %d x %d do not cover a %d x %d scene", n_y, n_x, kh, kw, H, W);
  const int bf16 = dtype == JSPSR_BF16;
  if (!jspsr::aligned4(out) || (reinterpret_cast<uintptr_t>(tiles) & (bf16 ? 1u : 3u)) || !jspsr::aligned4(wy) || !jspsr::aligned4(wx) ||
      !jspsr::aligned4(lo_y) || !jspsr::aligned4(lo_x) || !jspsr::aligned4(oy) || !jspsr::aligned4(ox) || !jspsr::aligned4(samples))
    return jspsr::fail(JSPSR_EALIGN, "scene_merge_windows: pointers not aligned to their element size");
  MergeArgs a{};
  a.tiles = tiles;
  a.wy = wy;
  a.wx = wx;
  a.lo_y = lo_y;
  a.lo_x = lo_x;
  a.oy = oy;
  a.ox = ox;
  a.samples = samples;
  a.out = out;
  a.bf16 = bf16;
  a.S = S;
  a.n_y = n_y;
  a.n_x = n_x;
  a.kh = kh;
  a.kw = kw;
  a.H = H;
  a.W = W;
  a.metres = metres ? 1 : 0;
  a.elev_log = elev_log ? 1 : 0;
  a.vec = (W & 3) == 0 && jspsr::aligned16(out);
  a.e = elev_range(elev_min, elev_max);
  const long long items = (long long)S * H * ((W + 3) / 4);
  hipLaunchKernelGGL(scene_merge_windows_kernel, dim3(blocks_for(items)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return jspsr::check_launch("scene_merge_windows");
}
