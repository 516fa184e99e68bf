// K16 -- the self-ensemble per window of a tiled scene (jspsr_amd/infer.py: prepare_windows_d4, predict_scenes(window_tta=...)):
//   jspsr_scene_prepare_windows_d4   K15's prepare_windows (scene_tiles.hip) composed with K14's D4 map (d4.h): a window AND a
//                                    D4 code per sample, the windows of a launch from any scenes of the store, ONE launch per
//                                    rot90 parity.  The bits of prepare_windows' output moved by the transform.
// The other side of the forwards is K14's jspsr_scene_finish_mean with the tile as its "scene" and K15's merge; nothing new.
//
// Output pixel (i, j) of sample b is ToTensor_kind of scene pixel (y0 + sy, x0 + sx), (sy, sx) = d4_source(code, kh, kw, i, j):
// the transform acts on the kh x kw window, the scene's own base, H and W enter the arithmetic (coord: the local coordinates
// of the source pixel over the whole scene), a source pixel outside its scene is NaN.
//
// Even rot90 (0, 2), output [B][cpitch][kh][kw]: an output row is a source row read forwards or backwards -- K15's streaming
// kernel with the indices taken through the map, four pixels per thread, no LDS.
//
// Odd rot90 (1, 3), output [B][cpitch][kw][kh]: an output ROW walks a source COLUMN, so an unstaged gather of the HWC store
// would stride by a whole scene row.  One workgroup makes one 32 x 32 output tile of one kind of one sample, as K14's
// scene_prepare_odd_kernel does.  There are no frame maps here: the tile's pre-image is exactly a block of tw rows x th
// columns of the window; clipped to the scene its rows are contiguous runs of at most 32 * 16 = 512 HWC bytes, read with
// coalesced dword loads (the aligned dwords that cover the run: 128 + 2 at most; byte-wise where a dword would straddle the
// end of the store) into K14's image
//   lds[32][kPitch],  kPitch = 131 dwords (odd), 16.4 KiB: nine workgroups fit a CU's 160 KiB, the 32-wave cap admits eight.
// Bank arithmetic of the read-out (K14's, the layout is unchanged): thread t owns output pixels (oy = t / 8, ox = 4 (t % 8) + p),
// p = 0..3; for one p the 32 lanes that a 4-byte or 1-byte LDS read serves together hold 4 values of oy = 4 consecutive source
// COLUMNS and 8 values of ox = 8 source ROWS four apart.  Rows four apart are 4 * 131 = 524 = 12 (mod 32) banks apart: the
// eight rows start in banks 0, 12, 24, 4, 16, 28, 8, 20, all distinct and four apart (an even pitch would put them all into
// one bank: 8-way).  The four columns add floor(col * pxb / 4) = 0..3 banks for the DEM (4 B a pixel) and the image (3 B):
// conflict-free; for a 15-channel mask (15 B a pixel: 0, 3, 7, 11) two of the 32 lanes can meet in a bank: 2-way at worst.
// Every staged pixel is inside the block by construction, so there is no read from the store in the read-out.
//
// All offsets into the store and the outputs are 64-bit, as in K15.
#include "common.h"
#include "d4.h"
#include "totensor.h"

#include <climits>
#include <cmath>

namespace {

using namespace jspsr;

constexpr int kTile = 32;                                   // output tile side
constexpr int kPitch = (kTile * kMaxC + 8) / 4 | 1;        // LDS row pitch in dwords: 32 px x 16 B + the unaligned head, odd

struct KindDesc {
  const unsigned char* src;   // scene store of this kind (HWC, C channels of 1 or 4 bytes); NULL for COORD
  long long src_bytes;
  float* out;                 // [B][cpitch][oh][ow]; this kind's channels start at coff
  int kind, C, coff, cpitch;
  int vec;                    // 16-byte stores: ow % 4 == 0 and out 16-byte aligned
};

struct WindowD4Args {
  KindDesc d[kKinds];         // the present kinds, packed
  const long long* scenes;    // [n_scenes][3] {pixel offset, H, W}
  const int* samples;         // [B][5] {scene, base (fp32 bits), y0, x0, code}
  int n_scenes, B, kh, kw, flags, mask_div;
  float lo, span;             // fp32(elev_min), fp32(elev_max - elev_min)
  double log_span;            // log(elev_max - elev_min)
};

int blocks_for(long long n) {
  long long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// The scene of sample row `row`: false unless it lies inside its store and the row's code has the launch's parity
__device__ __forceinline__ bool sample_scene(const WindowD4Args& a, const KindDesc& d, const int* row, int pxb, int parity,
                                             long long& off, long long& H, long long& W) {
  const int scene = row[0], code = row[4];
  off = 0; H = 0; W = 0;
  if (scene < 0 || scene >= a.n_scenes || code < 0 || code > 15 || ((code >> 2) & 1) != parity) return false;
  const long long o = a.scenes[scene * 3], h = a.scenes[scene * 3 + 1], w = a.scenes[scene * 3 + 2];
  if (o < 0 || h <= 0 || w <= 0 || h > INT_MAX || w > INT_MAX) return false;
  if (d.kind == COORD ? !(h > 1 && w > 1) : (o + h * w) * pxb > d.src_bytes) return false;
  off = o; H = h; W = w;
  return true;
}

// rot90 0 / 2: scene_prepare_windows_kernel (scene_tiles.hip), the window row and columns taken through the D4 map
__global__ __launch_bounds__(256) void scene_prepare_windows_even_kernel(WindowD4Args a) {
  const KindDesc& d = a.d[blockIdx.y];
  const int Wq = (a.kw + 3) >> 2;                                     // quads of an output row
  const long long total = (long long)a.B * a.kh * Wq;
  const int es = d.kind == LR_DEM ? 4 : 1;                            // bytes per channel value
  const int pxb = d.C * es;                                           // bytes per pixel
  const size_t plane = (size_t)a.kh * a.kw;
  const float nan = __int_as_float(0x7fc00000);
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int X = (int)(idx % Wq) * 4;
    const long long r = idx / Wq;
    const int Y = (int)(r % a.kh), b = (int)(r / a.kh);
    const int n = min(4, a.kw - X);
    const int* row = a.samples + (size_t)b * 5;
    const float base = __int_as_float(row[1]);
    const int code = row[4] & 11;                                     // an even angle whatever the table holds
    long long off, H, W;
    const bool ok = sample_scene(a, d, row, pxb, 0, off, H, W);
    int sy, sx;                                                       // the first of the four; the others lie in the same
    d4_source(code, a.kh, a.kw, Y, X, sy, sx);                        // window row, one column on or one column back
    const int step = ((code >> 3) ^ (code >> 1)) & 1 ? -1 : 1;        // a half turn or a mirror image, not both
    const long long ay = (long long)row[2] + sy;                      // scene row and columns; 64-bit: y0 and x0 are the caller's
    long long ax[4];
    bool okp[4];
    const unsigned char* p[4];
    for (int q = 0; q < 4; ++q) {
      ax[q] = (long long)row[3] + sx + step * min(q, n - 1);
      okp[q] = ok && ay >= 0 && ay < H && ax[q] >= 0 && ax[q] < W;
      p[q] = okp[q] && d.kind != COORD ? d.src + (off + ay * W + ax[q]) * pxb : nullptr;
    }
    float* o = d.out + ((size_t)b * d.cpitch + d.coff) * plane + (size_t)Y * a.kw + X;
    for (int c = 0; c < d.C; ++c, o += plane) {
      float v[4];
      for (int q = 0; q < 4; ++q) v[q] = okp[q] ? transform(d.kind, c, p[q] + c * es, base, (int)ay, (int)ax[q], H, W, a) : nan;
      if (d.vec) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        for (int q = 0; q < n; ++q) o[q] = v[q];
      }
    }
  }
}

// rot90 1 / 3: one 32 x 32 tile of the kw x kh output of one kind of one sample per workgroup, its pre-image staged in LDS
// (header)
__global__ __launch_bounds__(256) void scene_prepare_windows_odd_kernel(WindowD4Args a, int tiles_x) {
  __shared__ unsigned int lds[kTile * kPitch];
  __shared__ int rowoff[kTile];                               // LDS byte offset of block row r's first pixel
  const KindDesc& d = a.d[blockIdx.z];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int oh = a.kw, ow = a.kh;                                     // the transformed window
  const int Y0 = (blockIdx.x / tiles_x) * kTile, X0 = (blockIdx.x % tiles_x) * kTile;
  const int th = min(kTile, oh - Y0), tw = min(kTile, ow - X0);
  const int* row = a.samples + (size_t)b * 5;
  const float base = __int_as_float(row[1]);
  const int code = (row[4] & 15) | 4;                                 // an odd angle whatever the table holds
  const int es = d.kind == LR_DEM ? 4 : 1;                            // bytes per channel value
  const int pxb = d.C * es;                                           // bytes per pixel
  long long off, H, W;
  const bool ok = sample_scene(a, d, row, pxb, 1, off, H, W);         // !ok: H = W = 0, the block is empty

  // the tile's pre-image in the window: the D4 map is axis-aligned and monotonic, so two opposite corners span it -- tw
  // rows (an output column is a source row) by th columns; then in the scene, clipped to it
  int sya, sxa, syb, sxb;
  d4_source(code, a.kh, a.kw, Y0, X0, sya, sxa);
  d4_source(code, a.kh, a.kw, Y0 + th - 1, X0 + tw - 1, syb, sxb);
  const long long ay0 = (long long)row[2] + min(sya, syb), ax0 = (long long)row[3] + min(sxa, sxb);
  const long long cy0 = max(ay0, 0ll), cx0 = max(ax0, 0ll);
  const int nr = (int)max(min(ay0 + tw, H) - cy0, 0ll), nc = (int)max(min(ax0 + th, W) - cx0, 0ll);   // <= 32 each
  const int seg = nc * pxb;                                           // bytes per block row, <= 512
  if (tid < nr) rowoff[tid] = tid * kPitch * 4 + (int)((off + (cy0 + tid) * W + cx0) * pxb & 3);
  if (d.kind != COORD && nc > 0) {
    // stage: block row r = scene bytes [s, s + seg), read as the aligned dwords that cover it (bytes past the end of the
    // store are never touched: a dword that straddles it is read byte by byte), as K14 does
    const int ndw = seg / 4 + 2;                                      // <= kPitch
    for (int idx = tid; idx < nr * ndw; idx += 256) {
      const int r = idx / ndw, k = idx - r * ndw;
      const long long s = (off + (cy0 + r) * W + cx0) * pxb;
      const long long a0 = (s & ~3ll) + 4ll * k;
      if (a0 >= s + seg) continue;
      unsigned int v;
      if (a0 + 4 <= d.src_bytes) {
        v = *reinterpret_cast<const unsigned int*>(d.src + a0);
      } else {
        v = 0;
        for (int q = 0; q < 4; ++q)
          if (a0 + q < d.src_bytes) v |= (unsigned int)d.src[a0 + q] << (8 * q);
      }
      lds[r * kPitch + k] = v;
    }
  }
  __syncthreads();

  // thread tid owns output pixels (oy, ox .. ox + 3) of the tile in every channel: 32 rows x 8 groups of 4 = 256
  const int oy = tid >> 3, ox = (tid & 7) * 4;
  if (oy >= th || ox >= tw) return;
  const int n = min(4, tw - ox);
  const unsigned char* l8 = reinterpret_cast<const unsigned char*>(lds);
  int po[4], py[4], px[4];                                            // LDS byte offset, scene row, scene column
  bool okp[4];
  for (int p = 0; p < 4; ++p) {
    int sy, sx;
    d4_source(code, a.kh, a.kw, Y0 + oy, X0 + ox + min(p, n - 1), sy, sx);
    const long long ay = (long long)row[2] + sy, ax = (long long)row[3] + sx;
    okp[p] = ok && ay >= 0 && ay < H && ax >= 0 && ax < W;
    py[p] = okp[p] ? (int)ay : 0;
    px[p] = okp[p] ? (int)ax : 0;
    po[p] = okp[p] ? rowoff[(int)(ay - cy0)] + (int)(ax - cx0) * pxb : 0;      // inside the block: it is the pre-image
  }
  const size_t plane = (size_t)oh * ow;
  float* o = d.out + ((size_t)b * d.cpitch + d.coff) * plane + (size_t)(Y0 + oy) * ow + X0 + ox;
  for (int c = 0; c < d.C; ++c, o += plane) {
    float v[4];
    for (int p = 0; p < 4; ++p) {
      unsigned int raw = 0;                                           // the channel's bytes, from the staged block
      if (okp[p] && d.kind != COORD) {
        const unsigned char* l = l8 + po[p] + c * es;
        raw = es == 4 ? *reinterpret_cast<const unsigned int*>(l) : (unsigned int)*l;
      }
      v[p] = okp[p] ? transform(d.kind, c, reinterpret_cast<const unsigned char*>(&raw), base, py[p], px[p], H, W, a)
                    : __int_as_float(0x7fc00000);
    }
    if (d.vec) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int p = 0; p < n; ++p) o[p] = v[p];
    }
  }
}

}  // namespace

extern "C" int jspsr_scene_prepare_windows_d4(const void* const* src, const long long* src_bytes, float* const* out,
                                              const int* channels, const int* coff, const int* cpitch, const long long* scenes,
                                              int n_scenes, const int* samples, const int* codes, int B, int kh, int kw, int flags,
                                              double elev_min, double elev_max, int mask_div, jspsr_stream_t stream) {
  if (!src || !src_bytes || !out || !channels || !coff || !cpitch || !scenes || !samples || !codes || n_scenes <= 0 || B <= 0 ||
      kh <= 0 || kw <= 0 || !(elev_max > elev_min) || mask_div <= 0 || (flags & ~JSPSR_BATCH_FLAGS))
    return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: bad arguments");
  if (B > 65535) return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: %d samples, at most 65535 in a launch", B);
  if ((flags & JSPSR_BATCH_IMAGE_11) && (flags & JSPSR_BATCH_IMAGE_255))
    return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: image range [-1, 1] and [0, 255] together");
  if (out[HR_DEM]) return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: kind 1 (hr_dem) is not an input of the model");
  if (!jspsr::aligned4(samples) || (reinterpret_cast<uintptr_t>(scenes) & 7u))
    return jspsr::fail(JSPSR_EALIGN, "scene_prepare_windows_d4: tables not aligned to their element size");
  for (int b = 0; b < B; ++b) {
    if (codes[b] < 0 || codes[b] > 15)
      return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: sample %d: code %d outside 0..15", b, codes[b]);
    if (((codes[b] ^ codes[0]) >> 2) & 1)
      return jspsr::fail(JSPSR_EINVAL,
                         "scene_prepare_windows_d4: sample %d: rot90 %d beside rot90 %d, a launch holds one parity (one output shape)",
                         b, codes[b] >> 2, codes[0] >> 2);
  }
  const int odd = (codes[0] >> 2) & 1;
  const int oh = odd ? kw : kh, ow = odd ? kh : kw;                   // the transformed window
  WindowD4Args a{};
  int nk = 0;
  for (int kind = 0; kind < kKinds; ++kind) {
    if (!out[kind]) continue;
    const int C = channels[kind];
    const int need = kind == COORD ? 2 : (kind == IMAGE || kind == MASK) ? -1 : 1;
    if (C <= 0 || C > kMaxC || (need > 0 && C != need) || coff[kind] < 0 || cpitch[kind] < coff[kind] + C)
      return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: kind %d: bad channels (%d, offset %d, pitch %d)", kind, C, coff[kind],
                         cpitch[kind]);
    if (!jspsr::aligned4(out[kind]))
      return jspsr::fail(JSPSR_EALIGN, "scene_prepare_windows_d4: kind %d: output not 4-byte aligned", kind);
    if (kind != COORD) {
      if (!src[kind] || src_bytes[kind] <= 0)
        return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: kind %d: null or empty store", kind);
      if (!jspsr::aligned4(src[kind]))
        return jspsr::fail(JSPSR_EALIGN, "scene_prepare_windows_d4: kind %d: store not 4-byte aligned", kind);
    }
    a.d[nk++] = KindDesc{static_cast<const unsigned char*>(kind == COORD ? nullptr : src[kind]), kind == COORD ? 0 : src_bytes[kind],
                         out[kind], kind, C, coff[kind], cpitch[kind], (ow & 3) == 0 && jspsr::aligned16(out[kind])};
  }
  if (nk == 0) return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: no output");
  a.scenes = scenes;
  a.samples = samples;
  a.n_scenes = n_scenes;
  a.B = B;
  a.kh = kh;
  a.kw = kw;
  a.flags = flags;
  a.mask_div = mask_div;
  a.lo = (float)elev_min;                                   // the Python numbers, as numpy casts them against fp32 arrays
  a.span = (float)(elev_max - elev_min);
  a.log_span = log(elev_max - elev_min);
  if (odd) {
    const long long tiles_x = (ow + kTile - 1) / kTile, tiles = tiles_x * ((oh + kTile - 1) / kTile);
    if (tiles > INT_MAX) return jspsr::fail(JSPSR_EINVAL, "scene_prepare_windows_d4: a %d x %d window has too many tiles", kh, kw);
    hipLaunchKernelGGL(scene_prepare_windows_odd_kernel, dim3((unsigned)tiles, B, nk), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a, (int)tiles_x);
  } else {
    const long long items = (long long)B * kh * ((kw + 3) / 4);
    hipLaunchKernelGGL(scene_prepare_windows_even_kernel, dim3(blocks_for(items), nk), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a);
  }
  return jspsr::check_launch("scene_prepare_windows_d4");
}
