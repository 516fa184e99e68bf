// K14 -- whole-scene self-ensemble (the "+" of EDSR+): K13's two launches for the eight orientations of a scene.
//   jspsr_scene_prepare_d4   the D4 element of every sample, then add_padding + ToTensor: K13's gather through the frame maps
//                            of the TRANSFORMED shape, composed with K9's D4 map (code = angle * 4 + flip_lr * 2 + flip_ud)
//   jspsr_scene_finish_mean  the inverse transform of up to eight predictions, their fp32 mean in the order given, and K13's
//                            metre conversion, ONE launch
// A launch of prepare holds one parity of rot90, so one frame serves it.
//
// Even rot90 (0, 2): a frame row is a source row, read forwards or backwards -- K13's kernel with the indices reversed, no LDS.
//
// Odd rot90 (1, 3): a frame ROW walks a source COLUMN, so four consecutive frame pixels lie in four source rows and the HWC
// store would be read with a stride of a whole scene row.  One workgroup makes one 32 x 32 frame tile of one kind of one
// sample, as K9 does for its rotated crops.  The frame maps move by at most one source index per frame index (border and
// extension only reflect), so the tile's source pixels lie in a window of at most 32 x 32; its rows are contiguous runs of at
// most 32 * 16 = 512 HWC bytes, read with coalesced dword loads (the aligned dwords that cover the run: 128 + 2 at most) into
//   lds[32][kPitch],  kPitch = 131 dwords (odd), 16.4 KiB.
// Bank arithmetic of the read-out: thread t owns frame pixels (oy = t / 8, ox = 4 (t % 8) + p), p = 0..3; for one p the 32 lanes
// that an LDS read serves together hold 4 values of oy = 4 consecutive source COLUMNS and 8 values of ox = 8 source ROWS four
// apart.  Rows four apart are 4 * 131 = 524 = 12 (mod 32) banks apart: the eight rows start in banks 0, 12, 24, 4, 16, 28, 8,
// 20, all distinct and four apart (an even pitch would put them all into one bank: 8-way).  The four columns add
// floor(col * pxb / 4) = 0..3 banks for the DEM (4 B a pixel) and the image (3 B): conflict-free; for a 15-channel mask
// (15 B a pixel: 0, 3, 7, 11) two of the 32 lanes can meet in a bank: 2-way at worst.  The writes are the 16-byte runs of K13.
// A source pixel outside the staged window (maps that are not frame_maps') is read from the store directly.
//
// finish_mean: one workgroup makes one 32 x 32 tile of one scene's result.  An even variant's four pre-images are consecutive
// in a row of its prediction (forwards or backwards) and are read from memory directly, 128-byte runs per eight lanes.  An odd
// variant's lie in a column: its 32 x 32 tile of the prediction is staged with row-contiguous loads in lds[slot][32][33]
// (16.9 KiB: of eight distinct elements four are quarter turns, and the entry point refuses duplicates) and read transposed --
// pitch 33: lane (oy, ox) reads bank (ox + p + oy) mod 32 up to reflection, and within 32 lanes ox is a multiple of 4 and oy
// spans 4 values: conflict-free.
#include "common.h"
#include "d4.h"
#include "totensor.h"

#include <climits>
#include <cmath>

namespace {

using namespace jspsr;

constexpr int kTile = 32;                                   // frame / result tile side
constexpr int kPitch = (kTile * kMaxC + 8) / 4 | 1;        // LDS row pitch in dwords: 32 px x 16 B + the unaligned head, odd
constexpr int kPredPitch = kTile + 1;                       // floats
constexpr int kVariants = JSPSR_TTA_MAX_VARIANTS;
constexpr int kOddVariants = 4;                             // the quarter turns among eight distinct elements

struct KindDesc {
  const unsigned char* src;   // scene store of this kind (HWC, C channels of 1 or 4 bytes); NULL for COORD
  long long src_bytes;
  float* out;                 // [B][cpitch][Hp][Wp]; this kind's channels start at coff
  int kind, C, coff, cpitch;
  int vec;                    // 16-byte stores: Wp % 4 == 0 and out 16-byte aligned
};

struct PrepareArgs {
  KindDesc d[kKinds];         // the present kinds, packed
  const long long* scenes;    // [n_scenes][3] {pixel offset, H, W}
  const int* samples;         // [B][3] {scene, base (fp32 bits), code}
  const int* rows;            // [Hp] row of the TRANSFORMED scene at frame row Y
  const int* cols;            // [Wp] column of the transformed scene at frame column X
  int n_scenes, B, Hp, Wp, flags, mask_div;
  float lo, span;             // fp32(elev_min), fp32(elev_max - elev_min)
  double log_span;            // log(elev_max - elev_min)
};

struct Variant {
  const void* pred;           // [B][1][Hp][Wp]
  int bf16, code, Hp, Wp, top, left;
};

struct MeanArgs {
  Variant v[kVariants];
  float* out;                 // [B][H][W]
  const int* samples;         // [B][2] {scene, base (fp32 bits)}
  int K, B, H, W, metres, elev_log, vec;
  float lo, span, log_span, count;
};

int blocks_for(long long n) {
  long long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// d4_source / d4_image: the D4 index maps, shared with K16 (d4.h)

// The scene of sample row `row` ({scene, base, code}): false unless it lies inside its store and its code has the launch's parity
__device__ __forceinline__ bool sample_scene(const PrepareArgs& a, const KindDesc& d, const int* row, int pxb, int parity,
                                             long long& off, int& H, int& W) {
  const int scene = row[0], code = row[2];
  off = 0; H = 0; W = 0;
  if (scene < 0 || scene >= a.n_scenes || code < 0 || code > 15 || ((code >> 2) & 1) != parity) return false;
  const long long o = a.scenes[scene * 3], h = a.scenes[scene * 3 + 1], w = a.scenes[scene * 3 + 2];
  if (o < 0 || h <= 0 || w <= 0 || h > INT_MAX || w > INT_MAX) return false;
  if (d.kind == COORD ? !(h > 1 && w > 1) : (o + h * w) * pxb > d.src_bytes) return false;
  off = o; H = (int)h; W = (int)w;
  return true;
}

// rot90 0 / 2: K13's gather (scene.hip: scene_prepare_kernel), the source row and columns taken through the D4 map
__global__ __launch_bounds__(256) void scene_prepare_even_kernel(PrepareArgs a) {
  const KindDesc& d = a.d[blockIdx.y];
  const int Wq = (a.Wp + 3) >> 2;                                     // quads of a frame row
  const long long total = (long long)a.B * a.Hp * Wq;
  const int es = d.kind == LR_DEM ? 4 : 1;                            // bytes per channel value
  const int pxb = d.C * es;                                           // bytes per pixel
  const size_t plane = (size_t)a.Hp * a.Wp;
  const float nan = __int_as_float(0x7fc00000);
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int X = (int)(idx % Wq) * 4;
    const long long r = idx / Wq;
    const int Y = (int)(r % a.Hp), b = (int)(r / a.Hp);
    const int n = min(4, a.Wp - X);
    const int* row = a.samples + (size_t)b * 3;
    const float base = __int_as_float(row[1]);
    const int code = row[2] & 15;
    long long off;
    int H, W;
    bool ok = sample_scene(a, d, row, pxb, 0, off, H, W);
    const int i = a.rows[Y];
    ok = ok && i >= 0 && i < H;
    int sy = 0, sx[4];
    bool okp[4];
    const unsigned char* p[4];
    for (int q = 0; q < 4; ++q) {
      const int j = a.cols[X + min(q, n - 1)];
      int y, x;
      d4_source(code, H, W, i, j, y, x);
      okp[q] = ok && j >= 0 && j < W;
      sy = y;                                                         // the same for the four
      sx[q] = x;
      p[q] = okp[q] && d.kind != COORD ? d.src + (off + (long long)y * W + x) * pxb : nullptr;
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

// rot90 1 / 3: one 32 x 32 frame tile of one kind of one sample per workgroup, the source window staged in LDS (header)
__global__ __launch_bounds__(256) void scene_prepare_odd_kernel(PrepareArgs a, int tiles_x) {
  __shared__ unsigned int lds[kTile * kPitch];
  __shared__ int rowoff[kTile];                               // LDS byte offset of window row r's first pixel
  __shared__ int ti[kTile], tj[kTile];                        // transformed row / column of the tile's rows / columns, -1 = none
  __shared__ int win[4];                                      // their ranges: i min, i max, j min, j max
  const KindDesc& d = a.d[blockIdx.z];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int Y0 = (blockIdx.x / tiles_x) * kTile, X0 = (blockIdx.x % tiles_x) * kTile;
  const int th = min(kTile, a.Hp - Y0), tw = min(kTile, a.Wp - X0);
  const int* row = a.samples + (size_t)b * 3;
  const float base = __int_as_float(row[1]);
  const int code = (row[2] & 15) | 4;                                 // an odd angle whatever the table holds
  const int es = d.kind == LR_DEM ? 4 : 1;                            // bytes per channel value
  const int pxb = d.C * es;                                           // bytes per pixel
  long long off;
  int H, W;
  const bool ok = sample_scene(a, d, row, pxb, 1, off, H, W);         // !ok: H = W = 0 and no map entry is valid

  if (tid < 64) {                                                     // lanes 0..31 the tile's rows, 32..63 its columns
    const int t = tid & 31, isj = tid >> 5;
    int v = -1;
    if (t < (isj ? tw : th)) v = isj ? a.cols[X0 + t] : a.rows[Y0 + t];
    const bool in = v >= 0 && v < (isj ? H : W);                      // the transformed scene is W x H
    if (!in) v = -1;
    (isj ? tj : ti)[t] = v;
    int lo = in ? v : INT_MAX, hi = in ? v : INT_MIN;
    for (int m = 16; m; m >>= 1) {                                    // within each half of the wave
      lo = min(lo, __shfl_xor(lo, m));
      hi = max(hi, __shfl_xor(hi, m));
    }
    if (t == 0) { win[2 * isj] = lo; win[2 * isj + 1] = hi; }
  }
  __syncthreads();

  // the source window: the D4 map is axis-aligned and monotonic, so two opposite corners span it
  int sy0 = 0, sx0 = 0, nr = 0, nc = 0;
  if (win[0] <= win[1] && win[2] <= win[3]) {
    int sy1, sx1;
    d4_source(code, H, W, win[0], win[2], sy0, sx0);
    d4_source(code, H, W, win[1], win[3], sy1, sx1);
    if (sy0 > sy1) { const int t = sy0; sy0 = sy1; sy1 = t; }
    if (sx0 > sx1) { const int t = sx0; sx0 = sx1; sx1 = t; }
    nr = min(sy1 - sy0 + 1, kTile);
    nc = min(sx1 - sx0 + 1, kTile);
  }
  const int seg = nc * pxb;                                           // bytes per window row, <= 512
  if (tid < nr) rowoff[tid] = tid * kPitch * 4 + (int)((off + (long long)(sy0 + tid) * W + sx0) * pxb & 3);
  if (d.kind != COORD) {
    // stage: window row r = scene bytes [s, s + seg), read as the aligned dwords that cover it (bytes past the end of the
    // store are never touched: a dword that straddles it is read byte by byte), as K9 does
    const int ndw = seg / 4 + 2;                                      // <= kPitch
    for (int idx = tid; idx < nr * ndw; idx += 256) {
      const int r = idx / ndw, k = idx - r * ndw;
      const long long s = (off + (long long)(sy0 + r) * W + sx0) * pxb;
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

  // thread tid owns frame pixels (oy, ox .. ox + 3) of the tile in every channel: 32 rows x 8 groups of 4 = 256
  const int oy = tid >> 3, ox = (tid & 7) * 4;
  if (oy >= th || ox >= tw) return;
  const int n = min(4, tw - ox);
  const unsigned char* l8 = reinterpret_cast<const unsigned char*>(lds);
  const int i = ti[oy];
  int po[4], py[4], px[4];                                            // LDS byte offset (-1: not staged), scene row, column
  bool okp[4];
  for (int p = 0; p < 4; ++p) {
    const int j = tj[ox + min(p, n - 1)];
    okp[p] = ok && i >= 0 && j >= 0;
    py[p] = px[p] = 0;
    po[p] = -1;
    if (okp[p]) {
      d4_source(code, H, W, i, j, py[p], px[p]);
      const int r = py[p] - sy0, c = px[p] - sx0;
      if (r >= 0 && r < nr && c >= 0 && c < nc) po[p] = rowoff[r] + c * pxb;
    }
  }
  float* o = d.out + (((size_t)b * d.cpitch + d.coff) * a.Hp + Y0 + oy) * a.Wp + X0 + ox;
  const size_t plane = (size_t)a.Hp * a.Wp;
  for (int c = 0; c < d.C; ++c, o += plane) {
    float v[4];
    for (int p = 0; p < 4; ++p) {
      unsigned int raw = 0;                                           // the channel's bytes, from the tile or from the store
      if (okp[p] && d.kind != COORD) {
        if (po[p] >= 0) {
          const unsigned char* l = l8 + po[p] + c * es;
          raw = es == 4 ? *reinterpret_cast<const unsigned int*>(l) : (unsigned int)*l;
        } else {
          const unsigned char* g = d.src + (off + (long long)py[p] * W + px[p]) * pxb + c * es;
          raw = es == 4 ? *reinterpret_cast<const unsigned int*>(g) : (unsigned int)*g;
        }
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

__device__ __forceinline__ float load_pred(const void* p, size_t i, int bf16) {
  if (bf16) return __uint_as_float((unsigned int)static_cast<const unsigned short*>(p)[i] << 16);
  return static_cast<const float*>(p)[i];
}

// out[b][y][x] = post((((y'_0 + y'_1) + y'_2) + ...) / K), y'_k[y][x] = pred_k[b][top_k + i][left_k + j] with (i, j) the
// image of (y, x) under element k; post = scene_finish_kernel's expressions (scene.hip)
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
    float t = __fdiv_rn(acc[q], a.count);                             // K = 1: x / 1.0f is x
    if (a.metres) {
      t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
      t = a.elev_log ? __fadd_rn(expf(__fmul_rn(t, a.log_span)), a.lo) : __fadd_rn(__fmul_rn(t, a.span), a.lo);
      t = __fadd_rn(t, base);
    }
    r[q] = t;
  }
  float* o = a.out + ((size_t)b * a.H + y) * a.W + x0 + ox;
  if (a.vec) {
    *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
  } else {
    for (int q = 0; q < n; ++q) o[q] = r[q];
  }
}

// The element a code denotes, as the code with flip_ud clear: flipud = fliplr after a half turn
int canonical(int code) { return (code & 1) ? ((((code >> 2) + 2) & 3) << 2) | ((code & 2) ^ 2) : code; }

}  // namespace

extern "C" int jspsr_scene_prepare_d4(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                                      const int* coff, const int* cpitch, const long long* scenes, int n_scenes,
                                      const int* samples, const int* codes, int B, const int* rows, const int* cols, int Hp,
                                      int Wp, int flags, double elev_min, double elev_max, int mask_div, jspsr_stream_t stream) {
  if (!src || !src_bytes || !out || !channels || !coff || !cpitch || !scenes || !samples || !codes || !rows || !cols ||
      n_scenes <= 0 || B <= 0 || B > 65535 || Hp <= 0 || Wp <= 0 || !(elev_max > elev_min) || mask_div <= 0 ||
      (flags & ~JSPSR_BATCH_FLAGS))
    return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: bad arguments");
  if ((flags & JSPSR_BATCH_IMAGE_11) && (flags & JSPSR_BATCH_IMAGE_255))
    return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: image range [-1, 1] and [0, 255] together");
  if (out[HR_DEM]) return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: kind 1 (hr_dem) is not an input of the model");
  for (int b = 0; b < B; ++b) {
    if (codes[b] < 0 || codes[b] > 15)
      return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: sample %d: code %d outside 0..15", b, codes[b]);
    if (((codes[b] ^ codes[0]) >> 2) & 1)
      return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: sample %d: rot90 %d beside rot90 %d, a launch holds one parity (one frame)",
                         b, codes[b] >> 2, codes[0] >> 2);
  }
  const int odd = (codes[0] >> 2) & 1;
  PrepareArgs a{};
  int nk = 0;
  for (int kind = 0; kind < kKinds; ++kind) {
    if (!out[kind]) continue;
    const int C = channels[kind];
    const int need = kind == COORD ? 2 : (kind == IMAGE || kind == MASK) ? -1 : 1;
    if (C <= 0 || C > kMaxC || (need > 0 && C != need) || coff[kind] < 0 || cpitch[kind] < coff[kind] + C)
      return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: kind %d: bad channels (%d, offset %d, pitch %d)", kind, C, coff[kind], cpitch[kind]);
    if (!jspsr::aligned4(out[kind])) return jspsr::fail(JSPSR_EALIGN, "scene_prepare_d4: kind %d: output not 4-byte aligned", kind);
    if (kind != COORD) {
      if (!src[kind] || src_bytes[kind] <= 0) return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: kind %d: null or empty store", kind);
      if (!jspsr::aligned4(src[kind])) return jspsr::fail(JSPSR_EALIGN, "scene_prepare_d4: kind %d: store not 4-byte aligned", kind);
    }
    a.d[nk++] = KindDesc{static_cast<const unsigned char*>(kind == COORD ? nullptr : src[kind]), kind == COORD ? 0 : src_bytes[kind],
                         out[kind], kind, C, coff[kind], cpitch[kind], (Wp & 3) == 0 && jspsr::aligned16(out[kind])};
  }
  if (nk == 0) return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: no output");
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
  if (odd) {
    const long long tiles_x = (Wp + kTile - 1) / kTile, tiles = tiles_x * ((Hp + kTile - 1) / kTile);
    if (tiles > INT_MAX) return jspsr::fail(JSPSR_EINVAL, "scene_prepare_d4: a %d x %d frame has too many tiles", Hp, Wp);
    hipLaunchKernelGGL(scene_prepare_odd_kernel, dim3((unsigned)tiles, B, nk), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                       (int)tiles_x);
  } else {
    const long long items = (long long)B * Hp * ((Wp + 3) / 4);
    hipLaunchKernelGGL(scene_prepare_even_kernel, dim3(blocks_for(items), nk), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  }
  return jspsr::check_launch("scene_prepare_d4");
}

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
  // the constants as the reference's Python forms them (doubles), rounded once to the tensors' fp32 (jspsr_scene_finish)
  a.lo = (float)elev_min;
  a.span = (float)(elev_max - elev_min);
  a.log_span = (float)log(elev_max - elev_min);
  a.count = (float)K;
  const long long tiles_x = (W + kTile - 1) / kTile, tiles = tiles_x * ((H + kTile - 1) / kTile);
  if (tiles > INT_MAX) return jspsr::fail(JSPSR_EINVAL, "scene_finish_mean: a %d x %d scene has too many tiles", H, W);
  hipLaunchKernelGGL(scene_finish_mean_kernel, dim3((unsigned)tiles, B), dim3(256), 0, static_cast<hipStream_t>(stream), a,
                     (int)tiles_x);
  return jspsr::check_launch("scene_finish_mean");
}
