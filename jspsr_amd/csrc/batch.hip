// K9 -- the training batch, made on the device from a device-resident scene store (data/dfc30.py:193-246 + the transforms
// get_transformations chains, utils/common_config.py:112-161): RandomCrop / TileCrop's window, RandomFlipRotate90's D4 map
// (data/data_utils.py:9-30) and ToTensor's per-kind arithmetic (data_utils.py:217-312), for every raster of every sample of
// a batch in ONE launch.  HBM-bound: a 50 x 128^2 image + mask batch reads ~21 MB and writes ~65 MB.
//
// One workgroup makes one 32 x 32 output tile of one kind of one sample.  The tile's source window is a square of the
// scene (the D4 map sends an output tile to a square, transposed and / or mirrored); its rows are contiguous runs of HWC
// bytes, read with coalesced dword loads into LDS.  The D4 remap happens on the LDS read: the row pitch is an odd number of
// dwords, so the column walk of a rotated tile hits a different bank per row.  Each thread then writes four consecutive
// output pixels of a channel row at once (one 16-byte store when k % 4 == 0 and the output is 16-byte aligned).
#include "common.h"
#include "totensor.h"

#include <cmath>

namespace {

using namespace jspsr;                                      // Kind, kKinds, kMaxC, scale_dem, transform (totensor.h)

constexpr int kTile = 32;                                   // output tile side
constexpr int kPitch = (kTile * kMaxC + 8) / 4 | 1;        // LDS row pitch in dwords: 32 px x 16 B + the unaligned head, odd

struct KindDesc {
  const unsigned char* src;   // scene store of this kind (HWC, C channels of 1 or 4 bytes); NULL for COORD
  long long src_bytes;
  float* out;                 // [B][cpitch][k][k]; this kind's channels start at coff
  int kind, C, coff, cpitch;
  int vec;                    // 16-byte stores: k % 4 == 0 and out 16-byte aligned
};

struct BatchArgs {
  KindDesc d[kKinds];         // the present kinds, packed (gridDim.z of them)
  const long long* scenes;    // [n_scenes][3] {pixel offset, H, W}
  const int* samples;         // [B][8] {scene, y0, x0, code, base (fp32 bits), 0, 0, 0}
  int n_scenes, k, flags, mask_div;
  float lo, span;             // fp32(elev_min), fp32(elev_max - elev_min)
  double log_span;            // log(elev_max - elev_min), as the reference's np.log of a Python number
};

// Output (i, j) of a k x k crop -> crop position (sy, sx): the inverse of flipud(fliplr(rot90(crop, angle))) taken in
// the reference's order (rot90 first), code = angle * 4 + flip_lr * 2 + flip_ud.
__device__ __forceinline__ void d4_source(int code, int k, int i, int j, int& sy, int& sx) {
  const int i2 = (code & 1) ? k - 1 - i : i;
  const int j2 = (code & 2) ? k - 1 - j : j;
  switch (code >> 2) {
    case 0: sy = i2; sx = j2; break;
    case 1: sy = j2; sx = k - 1 - i2; break;          // np.rot90(m, 1)[i][j] = m[j][k-1-i]
    case 2: sy = k - 1 - i2; sx = k - 1 - j2; break;
    default: sy = k - 1 - j2; sx = i2; break;          // np.rot90(m, 3)[i][j] = m[k-1-j][i]
  }
}

// ToTensor, per kind (data_utils.py:217-312): scale_dem / transform of totensor.h, shared with K13-K16 (scene_prepare.hip)

__global__ __launch_bounds__(256) void batch_kernel(BatchArgs a, int tiles_x) {
  __shared__ unsigned int lds[kTile * kPitch];
  const KindDesc& d = a.d[blockIdx.z];
  const int b = blockIdx.y, tid = threadIdx.x, k = a.k;
  const int ty0 = (blockIdx.x / tiles_x) * kTile, tx0 = (blockIdx.x % tiles_x) * kTile;
  const int th = min(kTile, k - ty0), tw = min(kTile, k - tx0);
  const int* row = a.samples + (size_t)b * 8;
  const int scene = row[0], y0 = row[1], x0 = row[2], code = row[3];
  const float base = __int_as_float(row[4]);
  const int es = (d.kind == LR_DEM || d.kind == HR_DEM) ? 4 : 1;     // bytes per channel value
  const int pxb = d.C * es;                                           // bytes per pixel
  long long off = 0, H = 0, W = 0;
  bool ok = scene >= 0 && scene < a.n_scenes && code >= 0 && code < 16;
  if (ok) {
    off = a.scenes[scene * 3]; H = a.scenes[scene * 3 + 1]; W = a.scenes[scene * 3 + 2];
    ok = y0 >= 0 && x0 >= 0 && y0 + k <= H && x0 + k <= W && off >= 0 &&
         (d.kind == COORD ? H > 1 && W > 1 : (off + H * W) * pxb <= d.src_bytes);
  }
  // the tile's source window: the D4 map is axis-aligned, so two opposite output corners span it
  int sy0, sx0, sy1, sx1;
  d4_source(code & 15, k, ty0, tx0, sy0, sx0);
  d4_source(code & 15, k, ty0 + th - 1, tx0 + tw - 1, sy1, sx1);
  if (sy0 > sy1) { const int t = sy0; sy0 = sy1; sy1 = t; }
  if (sx0 > sx1) { const int t = sx0; sx0 = sx1; sx1 = t; }
  const int rows = sy1 - sy0 + 1, seg = (sx1 - sx0 + 1) * pxb;       // window rows, bytes per window row

  __shared__ int rowoff[kTile];                               // LDS byte offset of window row r's first pixel
  if (tid < rows) rowoff[tid] = tid * kPitch * 4 + (int)((off + (long long)(y0 + sy0 + tid) * W + x0 + sx0) * pxb & 3);
  if (ok && d.kind != COORD) {
    // stage: window row r = scene bytes [s, s + seg), read as the aligned dwords that cover it (bytes past either end of
    // the store are never touched: a dword that straddles one is read byte by byte)
    const int ndw = seg / 4 + 2;                                     // <= kPitch
    for (int idx = tid; idx < rows * ndw; idx += 256) {
      const int r = idx / ndw, i = idx - r * ndw;
      const long long s = (off + (long long)(y0 + sy0 + r) * W + x0 + sx0) * pxb;
      const long long a0 = (s & ~3ll) + 4ll * i;
      if (a0 >= s + seg) continue;
      unsigned int v;
      if (a0 + 4 <= d.src_bytes) {
        v = *reinterpret_cast<const unsigned int*>(d.src + a0);
      } else {
        v = 0;
        for (int q = 0; q < 4; ++q)
          if (a0 + q < d.src_bytes) v |= (unsigned int)d.src[a0 + q] << (8 * q);
      }
      lds[r * kPitch + i] = v;
    }
  }
  __syncthreads();

  // thread tid owns output pixels (oy, ox .. ox + 3) of the tile in every channel: 32 rows x 8 groups of 4 = 256
  const int oy = tid >> 3, ox = (tid & 7) * 4;
  if (oy >= th || ox >= tw) return;
  const int n = min(4, tw - ox);
  const unsigned char* l8 = reinterpret_cast<const unsigned char*>(lds);
  int po[4], py[4], px[4];                                            // LDS byte offset, scene row, scene column
  for (int p = 0; p < 4; ++p) {
    int sy, sx;
    d4_source(code & 15, k, ty0 + oy, tx0 + ox + min(p, n - 1), sy, sx);
    po[p] = rowoff[sy - sy0] + (sx - sx0) * pxb;
    py[p] = y0 + sy;
    px[p] = x0 + sx;
  }
  float* o = d.out + (((size_t)b * d.cpitch + d.coff) * k + ty0 + oy) * k + tx0 + ox;
  const size_t plane = (size_t)k * k;
  for (int c = 0; c < d.C; ++c, o += plane) {
    float v[4];
    for (int p = 0; p < 4; ++p)                                       // NaN marks a sample row outside its scene or store
      v[p] = ok ? transform(d.kind, c, l8 + po[p] + c * es, base, py[p], px[p], H, W, a) : __int_as_float(0x7fc00000);
    if (d.vec) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int p = 0; p < n; ++p) o[p] = v[p];
    }
  }
}

// K19 -- the validity plane of a batch: batch_kernel's sample rows and D4 map over a one-byte-per-pixel store, written as
// (B, 1, k, k) bytes, 1 = valid.  One workgroup makes one 32 x 32 tile of one sample.  Staged through LDS for the same
// reason as above: a quarter turn walks a COLUMN of the byte store, which read straight from global memory would cost one
// 64-byte request per output byte; instead the window's rows (runs of up to 32 bytes at any alignment) come in as the
// aligned dwords that cover them, and the column walk happens on the LDS read, over an odd dword pitch.  Each thread
// writes four consecutive output bytes (one dword store when k % 4 == 0 and the output is 4-byte aligned).
constexpr int kVPitch = (kTile + 8) / 4 | 1;                // 32 bytes + the unaligned head, odd: 11 dwords

__global__ __launch_bounds__(256) void batch_valid_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                         unsigned char* __restrict__ out,
                                                         const long long* __restrict__ scenes, int n_scenes,
                                                         const int* __restrict__ samples, int k, int tiles_x, int vec) {
  __shared__ unsigned int lds[kTile * kVPitch];
  __shared__ int rowoff[kTile];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * kTile, tx0 = (blockIdx.x % tiles_x) * kTile;
  const int th = min(kTile, k - ty0), tw = min(kTile, k - tx0);
  const int* row = samples + (size_t)b * 8;
  const int scene = row[0], y0 = row[1], x0 = row[2], code = row[3];
  long long off = 0, H = 0, W = 0;
  bool ok = scene >= 0 && scene < n_scenes && code >= 0 && code < 16;
  if (ok) {
    off = scenes[scene * 3]; H = scenes[scene * 3 + 1]; W = scenes[scene * 3 + 2];
    ok = y0 >= 0 && x0 >= 0 && y0 + k <= H && x0 + k <= W && off >= 0 && off + H * W <= src_bytes;
  }
  int sy0, sx0, sy1, sx1;
  d4_source(code & 15, k, ty0, tx0, sy0, sx0);
  d4_source(code & 15, k, ty0 + th - 1, tx0 + tw - 1, sy1, sx1);
  if (sy0 > sy1) { const int t = sy0; sy0 = sy1; sy1 = t; }
  if (sx0 > sx1) { const int t = sx0; sx0 = sx1; sx1 = t; }
  const int rows = sy1 - sy0 + 1, seg = sx1 - sx0 + 1;               // window rows (<= 32), bytes per window row (<= 32)
  if (tid < rows) rowoff[tid] = tid * kVPitch * 4 + (int)((off + (long long)(y0 + sy0 + tid) * W + x0 + sx0) & 3);
  if (ok) {
    const int ndw = seg / 4 + 2;                                     // <= 10 < kVPitch
    for (int idx = tid; idx < rows * ndw; idx += 256) {
      const int r = idx / ndw, i = idx - r * ndw;
      const long long s = off + (long long)(y0 + sy0 + r) * W + x0 + sx0;
      const long long a0 = (s & ~3ll) + 4ll * i;
      if (a0 >= s + seg) continue;
      unsigned int v;
      if (a0 + 4 <= src_bytes) {
        v = *reinterpret_cast<const unsigned int*>(src + a0);
      } else {                                                       // a dword that straddles the store's end: byte by byte
        v = 0;
        for (int q = 0; q < 4; ++q)
          if (a0 + q < src_bytes) v |= (unsigned int)src[a0 + q] << (8 * q);
      }
      lds[r * kVPitch + i] = v;
    }
  }
  __syncthreads();
  const int oy = tid >> 3, ox = (tid & 7) * 4;
  if (oy >= th || ox >= tw) return;
  const int n = min(4, tw - ox);
  const unsigned char* l8 = reinterpret_cast<const unsigned char*>(lds);
  unsigned int v[4];
  for (int p = 0; p < 4; ++p) {
    int sy, sx;
    d4_source(code & 15, k, ty0 + oy, tx0 + ox + min(p, n - 1), sy, sx);
    v[p] = ok ? (l8[rowoff[sy - sy0] + (sx - sx0)] != 0 ? 1u : 0u) : 0u;     // 0 marks a row outside its scene or store
  }
  unsigned char* o = out + ((size_t)b * k + ty0 + oy) * k + tx0 + ox;
  if (vec) {
    *reinterpret_cast<unsigned int*>(o) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
  } else {
    for (int p = 0; p < n; ++p) o[p] = (unsigned char)v[p];
  }
}

}  // namespace

extern "C" int jspsr_batch_valid(const unsigned char* store, long long store_bytes, unsigned char* out, const long long* scenes,
                                 int n_scenes, const int* samples, int B, int k, jspsr_stream_t stream) {
  if (!store || store_bytes <= 0 || !out || !scenes || !samples || n_scenes <= 0 || B <= 0 || k <= 0 || B > 65535)
    return jspsr::fail(JSPSR_EINVAL, "batch_valid: bad arguments");
  if (!jspsr::aligned4(store)) return jspsr::fail(JSPSR_EALIGN, "batch_valid: store not 4-byte aligned");
  const int tiles_x = (k + kTile - 1) / kTile;
  const int vec = (k & 3) == 0 && jspsr::aligned4(out);
  hipLaunchKernelGGL(batch_valid_kernel, dim3(tiles_x * tiles_x, B), dim3(256), 0, static_cast<hipStream_t>(stream), store,
                     store_bytes, out, scenes, n_scenes, samples, k, tiles_x, vec);
  return jspsr::check_launch("batch_valid");
}

extern "C" int jspsr_batch_make(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                                const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples,
                                int B, int k, int flags, double elev_min, double elev_max, int mask_div, jspsr_stream_t stream) {
  if (!src || !src_bytes || !out || !channels || !coff || !cpitch || !scenes || !samples || n_scenes <= 0 || B <= 0 || k <= 0 ||
      B > 65535 || !(elev_max > elev_min) || mask_div <= 0 || (flags & ~JSPSR_BATCH_FLAGS))
    return jspsr::fail(JSPSR_EINVAL, "batch_make: bad arguments");
  if ((flags & JSPSR_BATCH_IMAGE_11) && (flags & JSPSR_BATCH_IMAGE_255))
    return jspsr::fail(JSPSR_EINVAL, "batch_make: image range [-1, 1] and [0, 255] together");
  BatchArgs a{};
  int nk = 0;
  for (int kind = 0; kind < kKinds; ++kind) {
    if (!out[kind]) continue;
    const int C = channels[kind];
    const int need = kind == COORD ? 2 : (kind == IMAGE || kind == MASK) ? -1 : 1;
    if (C <= 0 || C > kMaxC || (need > 0 && C != need) || coff[kind] < 0 || cpitch[kind] < coff[kind] + C)
      return jspsr::fail(JSPSR_EINVAL, "batch_make: kind %d: bad channels (%d, offset %d, pitch %d)", kind, C, coff[kind], cpitch[kind]);
    if (!jspsr::aligned4(out[kind])) return jspsr::fail(JSPSR_EALIGN, "batch_make: kind %d: output not 4-byte aligned", kind);
    if (kind != COORD) {
      if (!src[kind] || src_bytes[kind] <= 0) return jspsr::fail(JSPSR_EINVAL, "batch_make: kind %d: null or empty store", kind);
      if (!jspsr::aligned4(src[kind])) return jspsr::fail(JSPSR_EALIGN, "batch_make: kind %d: store not 4-byte aligned", kind);
    }
    a.d[nk++] = KindDesc{static_cast<const unsigned char*>(kind == COORD ? nullptr : src[kind]), kind == COORD ? 0 : src_bytes[kind],
                         out[kind], kind, C, coff[kind], cpitch[kind], (k & 3) == 0 && jspsr::aligned16(out[kind])};
  }
  if (nk == 0) return jspsr::fail(JSPSR_EINVAL, "batch_make: no output");
  a.scenes = scenes;
  a.samples = samples;
  a.n_scenes = n_scenes;
  a.k = k;
  a.flags = flags;
  a.mask_div = mask_div;
  a.lo = (float)elev_min;                                   // the Python numbers, as numpy casts them against fp32 arrays
  a.span = (float)(elev_max - elev_min);
  a.log_span = log(elev_max - elev_min);
  const int tiles_x = (k + kTile - 1) / kTile;
  hipLaunchKernelGGL(batch_kernel, dim3(tiles_x * tiles_x, B, nk), dim3(256), 0, static_cast<hipStream_t>(stream), a, tiles_x);
  return jspsr::check_launch("batch_make");
}
