// K25 -- resampling single-channel fp32 rasters to a finer grid on the device: `F.interpolate(size=, mode="bicubic" |
// "bilinear", align_corners=False)` for a LIST of rasters of different shapes in one launch, so that a store can take its
// lr_dem at the resolution it is held in (30 m tiles under 8 m imagery: a ratio of 3.75) and the bicubic baseline of an
// evaluation needs no host.  Upsampling only (H >= h, W >= w): there is no prefilter here.
//
// (a) jspsr_resample_axis: the tap table of one axis, plain host code.  For output index Y of H over a source of h the
//     coordinate (Y + 0.5) h / H - 0.5 is taken apart in integers: n = (2Y + 1) h - H, d = 2H, i = floor(n / d), r = n - i d,
//     t = r / d in double -- no rounding at lattice points, H == h gives t = 0 exactly.  The cubic convolution weights
//     (A = -0.75, torch's and cv2's INTER_CUBIC) are evaluated in DOUBLE and rounded to fp32 once each: formed in fp32 they
//     cancel, their sum misses 1 by several ulp and a raster at 1500 m moves by a millimetre.
// (b) jspsr_resample_forward: one launch.  blockIdx.y is the raster, blockIdx.x its TH x TW output tile (a raster with
//     fewer tiles than the largest of the call leaves the rest of its row of the grid at once).  A workgroup stages the
//     tile's source patch in LDS with its indices already clamped to the raster (at most (TH + 3) x (TW + 3) values; at a
//     ratio of 3.75 a 21 x 21 patch under 4096 outputs).  A lane owns one output column: its four x weights stay in
//     registers, and it walks 16 output rows downwards; a row's taps are the same for the whole wave and come through
//     scalar loads, the weights as scalar operands.  Output rows that share their source row
//     i share the centre tap c and the four horizontal sums r_k, which are computed once per run of such rows (16 LDS
//     reads per 3.75 outputs); each row then costs four products and four sums.  A wave stores whole 256-byte row pieces.
//     The arithmetic interpolates the DIFFERENCES to the centre tap, using sum(w) = 1:
//         c   = v[clamp(iy)][clamp(ix)]
//         r_k = ((wx0 (v_k0 - c) + wx1 (v_k1 - c)) + wx2 (v_k2 - c)) + wx3 (v_k3 - c)          k = 0 .. 3
//         s   = ((wy0 r_0 + wy1 r_1) + wy2 r_2) + wy3 r_3
//         out = s + c, then out < lo ? lo : (out > hi ? hi : out) where a clamp is given (a NaN stays a NaN)
//     so the rounding errors scale with the relief under the taps and not with the elevation.  Every operation is ONE fp32
//     rounding: explicit __fsub_rn / __fmul_rn / __fadd_rn and -ffp-contract=off (csrc/Makefile), no fused multiply-add --
//     tests/resample_ref.py restates it in numpy float32 and the output has its bits, whatever rasters share the call.
//     Bilinear is the same form over its 2 x 2 taps with the first tap as the centre.
//     With a void plane the destination byte is the source byte of pixel (clamp(iy), clamp(ix)), written in the same launch.
// Nothing synchronises with the host, and no workspace is needed.
#include "common.h"

#include <cmath>

namespace {

using namespace jspsr;

constexpr int TH = 64, TW = 64;               // output tile of a workgroup
constexpr int NTHREADS = 256;                 // 4 waves: a lane per column, a wave per band of RW rows
constexpr int RW = TH / (NTHREADS / 64);      // rows a lane walks
constexpr int PH = TH + 3, PW = TW + 3;       // the largest source patch of a tile (H >= h: a step of at most one source pixel)
constexpr int ROW = 8;                        // table words per raster

template <int NT>
struct Mode;
template <>
struct Mode<4> { static constexpr int centre = 1; };       // bicubic: taps i-1 .. i+2
template <>
struct Mode<2> { static constexpr int centre = 0; };       // bilinear: taps i, i+1

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int NT, bool VOID>
__global__ __launch_bounds__(NTHREADS) void resample_kernel(const float* __restrict__ src, const long long* __restrict__ table,
                                                            const int* __restrict__ first, const float* __restrict__ weights,
                                                            const float* __restrict__ clampv, const unsigned char* __restrict__ svoid,
                                                            unsigned char* __restrict__ dvoid, float* __restrict__ dst) {
  constexpr int CT = Mode<NT>::centre;
  __shared__ float patch[PH][PW];
  const long long* __restrict__ row = table + (size_t)blockIdx.y * ROW;
  const long long src_off = row[0], dst_off = row[3], ytaps = row[6], xtaps = row[7];
  const int h = (int)row[1], w = (int)row[2], H = (int)row[4], W = (int)row[5];
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;              // workgroup-uniform: this raster has fewer tiles
  const int tid = threadIdx.x;
  const int Y0 = ((int)blockIdx.x / tiles_x) * TH, X0 = ((int)blockIdx.x % tiles_x) * TW;
  const int th = H - Y0 < TH ? H - Y0 : TH, tw = W - X0 < TW ? W - X0 : TW;
  const int fy0 = first[ytaps + Y0], fx0 = first[xtaps + X0];
  int ph = first[ytaps + Y0 + th - 1] + NT - fy0, pw = first[xtaps + X0 + tw - 1] + NT - fx0;
  ph = clampi(ph, 1, PH);                                        // a consistent table never needs these
  pw = clampi(pw, 1, PW);
  // the lane's column: its taps are asked for before the patch, so that they arrive with it
  const int lx = tid & 63, X = X0 + (lx < tw ? lx : tw - 1);     // a lane past the raster's edge reads the last column's taps
  const int fxg = first[xtaps + X];
  const float4 wx4 = *reinterpret_cast<const float4*>(weights + (xtaps + X) * 4);     // the entry checks the 16-byte alignment
  const float* __restrict__ s = src + src_off;
  for (int idx = tid; idx < ph * pw; idx += NTHREADS) {
    const int p = idx / pw, q = idx - p * pw;
    const int sy = clampi(fy0 + p, 0, h - 1), sx = clampi(fx0 + q, 0, w - 1);
    patch[p][q] = s[(long long)sy * w + sx];
  }
  __syncthreads();
  if (lx >= tw) return;                                          // no barrier follows
  const int fx = clampi(fxg - fx0, 0, PW - NT);
  const float wxa[4] = {wx4.x, wx4.y, wx4.z, wx4.w};
  float wx[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) wx[j] = wxa[j];
  const int cxs = clampi(fxg + CT, 0, w - 1);                    // the source column of the centre tap
  float lo = 0.f, hi = 0.f;
  const bool clamped = clampv != nullptr;
  if (clamped) {
    lo = clampv[2 * blockIdx.y];
    hi = clampv[2 * blockIdx.y + 1];
  }
  // the rows' taps are the same for every lane of a wave: scalar loads, scalar branches, weights as scalar operands
  const int yb = __builtin_amdgcn_readfirstlane(tid >> 6) * RW, ye = yb + RW < th ? yb + RW : th;
  const int* __restrict__ yf = first + ytaps + Y0;
  const float4* __restrict__ yw4 = reinterpret_cast<const float4*>(weights + (ytaps + Y0) * 4);
  int cur = -0x7fffffff;                                         // the source row the sums below belong to
  float c = 0.f, r[NT];
  unsigned char vbyte = 0;
  for (int y = yb; y < ye; ++y) {
    const int fy = yf[y];
    const float4 wy4 = yw4[y];
    const float yw[4] = {wy4.x, wy4.y, wy4.z, wy4.w};
    if (fy != cur) {
      cur = fy;
      const int py = clampi(fy - fy0, 0, PH - NT);
      c = patch[py + CT][fx + CT];
#pragma unroll
      for (int k = 0; k < NT; ++k) {
        float acc = __fmul_rn(wx[0], __fsub_rn(patch[py + k][fx], c));
#pragma unroll
        for (int j = 1; j < NT; ++j) acc = __fadd_rn(acc, __fmul_rn(wx[j], __fsub_rn(patch[py + k][fx + j], c)));
        r[k] = acc;
      }
      if constexpr (VOID) vbyte = svoid[src_off + (long long)clampi(fy + CT, 0, h - 1) * w + cxs];
    }
    float acc = __fmul_rn(yw[0], r[0]);
#pragma unroll
    for (int k = 1; k < NT; ++k) acc = __fadd_rn(acc, __fmul_rn(yw[k], r[k]));
    float out = __fadd_rn(acc, c);
    if (clamped) out = out < lo ? lo : (out > hi ? hi : out);    // both comparisons fail for a NaN
    const long long o = dst_off + (long long)(Y0 + y) * W + X;
    dst[o] = out;
    if constexpr (VOID) dvoid[o] = vbyte;
  }
}

// floor(n / d) and the remainder for d > 0
inline void floor_div(long long n, long long d, long long& i, long long& r) {
  i = n / d;
  r = n - i * d;
  if (r < 0) {
    --i;
    r += d;
  }
}

}  // namespace

extern "C" int jspsr_resample_axis(int h, int H, int mode, int* first, float* weights) {
  if (!first || !weights) return fail(JSPSR_EINVAL, "resample_axis: null pointer");
  if (mode != JSPSR_RESAMPLE_BICUBIC && mode != JSPSR_RESAMPLE_BILINEAR) return fail(JSPSR_EINVAL, "resample_axis: mode %d", mode);
  if (h < 1 || H < h) return fail(JSPSR_EINVAL, "resample_axis: %d -> %d (a source of at least one pixel, and no downsampling: H >= h)", h, H);
  const double A = -0.75;
  const long long d = 2ll * H;
  for (int Y = 0; Y < H; ++Y) {
    long long n = (2ll * Y + 1) * h - H, i, r;
    float* wr = weights + (size_t)Y * 4;
    if (mode == JSPSR_RESAMPLE_BILINEAR) {
      if (n < 0) n = 0;                                          // torch's clamp of the coordinate: i = 0, t = 0
      floor_div(n, d, i, r);
      const double t = (double)r / (double)d;
      first[Y] = (int)i;
      wr[0] = (float)(1.0 - t);
      wr[1] = (float)t;
      wr[2] = wr[3] = 0.f;
      continue;
    }
    floor_div(n, d, i, r);
    const double t = (double)r / (double)d;
    auto c1 = [A](double x) { return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0; };
    auto c2 = [A](double x) { return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A; };
    first[Y] = (int)i - 1;
    wr[0] = (float)c2(t + 1.0);
    wr[1] = (float)c1(t);
    wr[2] = (float)c1(1.0 - t);
    wr[3] = (float)c2(2.0 - t);
  }
  return JSPSR_OK;
}

extern "C" int jspsr_resample_forward(const float* src, long long src_numel, float* dst, long long dst_numel, const long long* table,
                                      const long long* host_table, int n, const int* first, const float* weights, long long n_taps,
                                      int mode, const float* clamp, const unsigned char* src_void, unsigned char* dst_void,
                                      jspsr_stream_t stream) {
  const char* const name = "resample_forward";
  if (!src || !dst || !table || !host_table || !first || !weights) return fail(JSPSR_EINVAL, "%s: null pointer", name);
  if (mode != JSPSR_RESAMPLE_BICUBIC && mode != JSPSR_RESAMPLE_BILINEAR) return fail(JSPSR_EINVAL, "%s: mode %d", name, mode);
  if (n < 1 || n > 65535) return fail(JSPSR_EINVAL, "%s: %d rasters, one call takes 1..65535", name, n);
  if ((src_void == nullptr) != (dst_void == nullptr)) return fail(JSPSR_EINVAL, "%s: a void plane needs its source and its destination", name);
  if (!aligned4(src) || !aligned4(dst) || !aligned4(first) || (clamp && !aligned4(clamp)))
    return fail(JSPSR_EALIGN, "%s: tensors not 4-byte aligned", name);
  if (!aligned16(weights)) return fail(JSPSR_EALIGN, "%s: weights not 16-byte aligned", name);      // a row of four is one load
  if (reinterpret_cast<uintptr_t>(table) & 7u) return fail(JSPSR_EALIGN, "%s: table not 8-byte aligned", name);
  long long max_tiles = 0;
  for (int k = 0; k < n; ++k) {                                  // every index the kernel forms stays inside the buffers
    const long long* r = host_table + (size_t)k * ROW;
    const long long so = r[0], h = r[1], w = r[2], dof = r[3], H = r[4], W = r[5], yt = r[6], xt = r[7];
    if (h < 1 || w < 1 || H < h || W < w || H > 0x3fffffff || W > 0x3fffffff)
      return fail(JSPSR_EINVAL, "%s: raster %d is %lld x %lld -> %lld x %lld (no empty side, no downsampling)", name, k, h, w, H, W);
    if (so < 0 || h * w > src_numel - so || dof < 0 || H * W > dst_numel - dof)
      return fail(JSPSR_EINVAL, "%s: raster %d leaves its buffer (source %lld + %lld of %lld, destination %lld + %lld of %lld)", name, k,
                  so, h * w, src_numel, dof, H * W, dst_numel);
    if (yt < 0 || H > n_taps - yt || xt < 0 || W > n_taps - xt)
      return fail(JSPSR_EINVAL, "%s: raster %d reads taps %lld + %lld and %lld + %lld of %lld", name, k, yt, H, xt, W, n_taps);
    const long long tiles = ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
    if (tiles > 0xffffff) return fail(JSPSR_EINVAL, "%s: raster %d has %lld tiles", name, k, tiles);   // 2^24 workgroups of 256 threads in x
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)max_tiles, (unsigned)n);
#define JSPSR_RESAMPLE_LAUNCH(NT, VOID)                                                                                            \
  hipLaunchKernelGGL((resample_kernel<NT, VOID>), grid, dim3(NTHREADS), 0, s, src, table, first, weights, clamp, src_void, dst_void, dst)
  if (mode == JSPSR_RESAMPLE_BICUBIC) {
    if (src_void) JSPSR_RESAMPLE_LAUNCH(4, true);
    else JSPSR_RESAMPLE_LAUNCH(4, false);
  } else {
    if (src_void) JSPSR_RESAMPLE_LAUNCH(2, true);
    else JSPSR_RESAMPLE_LAUNCH(2, false);
  }
#undef JSPSR_RESAMPLE_LAUNCH
  return check_launch(src_void ? "resample (void)" : "resample");
}
