// K13 -- whole-scene inference, the steps either side of the forward (upscale_dem, utils/utils.py:1556-1654):
//   jspsr_scene_prepare   add_padding (utils.py:1501-1520) + ToTensor (data/data_utils.py:217-312) of every raster of a
//                         batch of equally sized scenes, from the raw HWC scene store to the model's NCHW inputs, ONE launch
//   jspsr_scene_finish    remove_padding (utils.py:1523-1531) and, for metres, clip -> descale_data -> + base
//                         (evaluation/evaluate_utils.py:242-271), ONE launch
// Both are HBM streaming and writes dominate (prepare: 76 B written per frame pixel of image + mask against 22 B read per
// source pixel; finish: 4 B in, 4 B out).  No LDS: a thread makes four consecutive pixels of a frame row in every channel
// of its kind, so a wave writes 1 KiB runs of a channel plane (16-byte stores when Wp % 4 == 0 and the plane is 16-byte
// aligned) and its byte reads of the HWC store fall into the cache lines its neighbours read.
//
// The geometry is two int32 maps made on the host (jspsr_amd/infer.py: frame_maps): out[b][c][Y][X] =
// ToTensor(src[rows[Y]][cols[X]][c]).  add_padding's mirror border is separable, so the maps carry it index for index,
// and the extension to a multiple of the model's stride and plain cropping as well; the kernel is a gather fused with the
// per-kind arithmetic of totensor.h (K9's, bit for bit).  A map entry outside its scene writes NaN; nothing is read there.
#include "common.h"
#include "totensor.h"

#include <cmath>

namespace {

using namespace jspsr;

struct KindDesc {
  const unsigned char* src;   // scene store of this kind (HWC, C channels of 1 or 4 bytes); NULL for COORD
  long long src_bytes;
  float* out;                 // [B][cpitch][Hp][Wp]; this kind's channels start at coff
  int kind, C, coff, cpitch;
  int vec;                    // 16-byte stores: Wp % 4 == 0 and out 16-byte aligned
};

struct SceneArgs {
  KindDesc d[kKinds];         // the present kinds, packed (gridDim.y of them)
  const long long* scenes;    // [n_scenes][3] {pixel offset, H, W}
  const int* samples;         // [B][2] {scene, base (fp32 bits)}
  const int* rows;            // [Hp] source row of frame row Y
  const int* cols;            // [Wp] source column of frame column X
  int n_scenes, B, Hp, Wp, flags, mask_div;
  float lo, span;             // fp32(elev_min), fp32(elev_max - elev_min)
  double log_span;            // log(elev_max - elev_min)
};

int blocks_for(long long n) {
  long long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

__global__ __launch_bounds__(256) void scene_prepare_kernel(SceneArgs a) {
  const KindDesc& d = a.d[blockIdx.y];
  const int Wq = (a.Wp + 3) >> 2;                                     // quads of a frame row
  const long long total = (long long)a.B * a.Hp * Wq;
  const int es = d.kind == LR_DEM ? 4 : 1;                            // bytes per channel value
  const int pxb = d.C * es;                                           // bytes per pixel
  const size_t plane = (size_t)a.Hp * a.Wp;
  const float nan = __int_as_float(0x7fc00000);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int X = (int)(i % Wq) * 4;
    const long long r = i / Wq;
    const int Y = (int)(r % a.Hp), b = (int)(r / a.Hp);
    const int n = min(4, a.Wp - X);
    const int scene = a.samples[2 * b];
    const float base = __int_as_float(a.samples[2 * b + 1]);
    long long off = 0, H = 0, W = 0;
    bool ok = scene >= 0 && scene < a.n_scenes;
    if (ok) {
      off = a.scenes[scene * 3]; H = a.scenes[scene * 3 + 1]; W = a.scenes[scene * 3 + 2];
      ok = off >= 0 && H > 0 && W > 0 && (d.kind == COORD ? H > 1 && W > 1 : (off + H * W) * pxb <= d.src_bytes);
    }
    const int sy = a.rows[Y];
    ok = ok && sy >= 0 && sy < H;
    int sx[4];
    bool okp[4];
    const unsigned char* p[4];
    for (int q = 0; q < 4; ++q) {
      sx[q] = a.cols[X + min(q, n - 1)];
      okp[q] = ok && sx[q] >= 0 && sx[q] < W;
      p[q] = okp[q] && d.kind != COORD ? d.src + (off + (long long)sy * W + sx[q]) * pxb : nullptr;
    }
    float* o = d.out + ((size_t)b * d.cpitch + d.coff) * plane + (size_t)Y * a.Wp + X;
    for (int c = 0; c < d.C; ++c, o += plane) {
      float v[4];
      for (int q = 0; q < 4; ++q) v[q] = okp[q] ? transform(d.kind, c, p[q] + c * es, base, sy, sx[q], H, W, a) : nan;
      if (d.vec) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        for (int q = 0; q < n; ++q) o[q] = v[q];
      }
    }
  }
}

__device__ __forceinline__ float load_pred(const void* p, size_t i, int bf16) {
  if (bf16) return __uint_as_float((unsigned int)static_cast<const unsigned short*>(p)[i] << 16);
  return static_cast<const float*>(p)[i];
}

// out[b][y][x] = pred[b][top + y][left + x], in metres: clamp (a NaN stays a NaN, as torch.clamp leaves it), descale_data's
// two roundings, + base -- elev_scale_kernel's expressions (csrc/tiles.hip), the bits of summary.compose_scene
__global__ __launch_bounds__(256) void scene_finish_kernel(const void* __restrict__ pred, float* __restrict__ out,
                                                          const int* __restrict__ samples, int bf16, int B, int Hp, int Wp,
                                                          int top, int left, int H, int W, int metres, int elev_log, float lo,
                                                          float span, float log_span, int vec) {
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
      float t = load_pred(pred, s + min(q, n - 1), bf16);
      if (metres) {
        t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
        t = elev_log ? __fadd_rn(expf(__fmul_rn(t, log_span)), lo) : __fadd_rn(__fmul_rn(t, span), lo);
        t = __fadd_rn(t, base);
      }
      v[q] = t;
    }
    float* o = out + ((size_t)b * H + y) * W + x;
    if (vec) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int q = 0; q < n; ++q) o[q] = v[q];
    }
  }
}

}  // namespace

extern "C" int jspsr_scene_prepare(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                                   const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples,
                                   int B, const int* rows, const int* cols, int Hp, int Wp, int flags, double elev_min,
                                   double elev_max, int mask_div, jspsr_stream_t stream) {
  if (!src || !src_bytes || !out || !channels || !coff || !cpitch || !scenes || !samples || !rows || !cols || n_scenes <= 0 ||
      B <= 0 || Hp <= 0 || Wp <= 0 || !(elev_max > elev_min) || mask_div <= 0 || (flags & ~JSPSR_BATCH_FLAGS))
    return jspsr::fail(JSPSR_EINVAL, "scene_prepare: bad arguments");
  if ((flags & JSPSR_BATCH_IMAGE_11) && (flags & JSPSR_BATCH_IMAGE_255))
    return jspsr::fail(JSPSR_EINVAL, "scene_prepare: image range [-1, 1] and [0, 255] together");
  if (out[HR_DEM]) return jspsr::fail(JSPSR_EINVAL, "scene_prepare: kind 1 (hr_dem) is not an input of the model");
  SceneArgs a{};
  int nk = 0;
  for (int kind = 0; kind < kKinds; ++kind) {
    if (!out[kind]) continue;
    const int C = channels[kind];
    const int need = kind == COORD ? 2 : (kind == IMAGE || kind == MASK) ? -1 : 1;
    if (C <= 0 || C > kMaxC || (need > 0 && C != need) || coff[kind] < 0 || cpitch[kind] < coff[kind] + C)
      return jspsr::fail(JSPSR_EINVAL, "scene_prepare: kind %d: bad channels (%d, offset %d, pitch %d)", kind, C, coff[kind], cpitch[kind]);
    if (!jspsr::aligned4(out[kind])) return jspsr::fail(JSPSR_EALIGN, "scene_prepare: kind %d: output not 4-byte aligned", kind);
    if (kind != COORD) {
      if (!src[kind] || src_bytes[kind] <= 0) return jspsr::fail(JSPSR_EINVAL, "scene_prepare: kind %d: null or empty store", kind);
      if (!jspsr::aligned4(src[kind])) return jspsr::fail(JSPSR_EALIGN, "scene_prepare: kind %d: store not 4-byte aligned", kind);
    }
    a.d[nk++] = KindDesc{static_cast<const unsigned char*>(kind == COORD ? nullptr : src[kind]), kind == COORD ? 0 : src_bytes[kind],
                         out[kind], kind, C, coff[kind], cpitch[kind], (Wp & 3) == 0 && jspsr::aligned16(out[kind])};
  }
  if (nk == 0) return jspsr::fail(JSPSR_EINVAL, "scene_prepare: no output");
  a.scenes = scenes;
  a.samples = samples;
  a.rows = rows;
  a.cols = cols;
  a.n_scenes = n_scenes;
  a.B = B;
  a.Hp = Hp;
  a.Wp = Wp;
  a.flags = flags;
  a.mask_div = mask_div;
  a.lo = (float)elev_min;                                   // the Python numbers, as numpy casts them against fp32 arrays
  a.span = (float)(elev_max - elev_min);
  a.log_span = log(elev_max - elev_min);
  const long long items = (long long)B * Hp * ((Wp + 3) / 4);
  hipLaunchKernelGGL(scene_prepare_kernel, dim3(blocks_for(items), nk), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return jspsr::check_launch("scene_prepare");
}

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
  // the constants as the reference's Python forms them (doubles), rounded once to the tensors' fp32 (jspsr_elev_scale_f32)
  const float span = (float)(elev_max - elev_min);
  const float log_span = (float)log(elev_max - elev_min);
  const long long items = (long long)B * H * ((W + 3) / 4);
  hipLaunchKernelGGL(scene_finish_kernel, dim3(blocks_for(items)), dim3(256), 0, static_cast<hipStream_t>(stream), pred, out, samples,
                     bf16, B, Hp, Wp, top, left, H, W, metres ? 1 : 0, elev_log ? 1 : 0, (float)elev_min, span, log_span,
                     (W & 3) == 0 && jspsr::aligned16(out));
  return jspsr::check_launch("scene_finish");
}
