// K13-K16 -- prepare: the raw HWC scene store -> the model's fp32 NCHW inputs (add_padding, utils/utils.py:1501-1520, and
// ToTensor, data/data_utils.py:217-312, of every raster), ONE launch per entry (per rot90 parity with a D4 code):
//   jspsr_scene_prepare              K13  whole scenes through the frame maps (jspsr_amd/infer.py: frame_maps)
//   jspsr_scene_prepare_d4           K14  the D4 element of every sample, then K13's frame of the TRANSFORMED shape
//   jspsr_scene_prepare_windows      K15  kh x kw windows of any scenes of the store
//   jspsr_scene_prepare_windows_d4   K16  a window AND a D4 element per sample: K15's bits moved by the transform
// code = rot90 * 4 + flip_lr * 2 + flip_ud (d4.h).  A source pixel outside its scene writes NaN; nothing is read there.
// All offsets into the store and the outputs are 64-bit: a 37 000 x 37 000 scene's image plane passes 2^31 bytes.
//
// Structure.  Two kernel templates, parameterised at compile time by the GEOMETRY -- how output pixel (Y, X) of a sample
// becomes a source pixel: `Frames` (two int32 maps, out[Y][X] = scene'[rows[Y]][cols[X]]; add_padding's mirror border is
// separable, so the maps carry it and the extension to the model's stride index for index) or `Windows` (an origin
// (y0, x0) per sample) -- and by whether a D4 code is read.  The geometry is the only policy; the argument block and its
// validation, the scene lookup, the staging, the read-out and the per-kind epilogue are shared (scene_prepare.h).  The
// upright entries are instantiations WITHOUT a code, not the D4 kernel run with code 0: decoding the element at run time
// costs the streaming kernel 5-23 % (profiles/r12_tta_bench.txt, profiles/r15_window_tta_bench.txt).
//
// stream_kernel (upright, and rot90 0 / 2: an output row is a source row, read forwards or backwards).  HBM streaming,
// writes dominate (76 B written per output pixel of image + mask against 22 B read per source pixel).  No LDS: a thread
// makes four consecutive pixels of an output row in every channel of its kind, so a wave writes 1 KiB runs of a channel
// plane (16-byte stores when Wp % 4 == 0 and the plane is 16-byte aligned) and its byte reads of the HWC store fall into
// the cache lines its neighbours read.
//
// staged_kernel (rot90 1 / 3): an output ROW walks a source COLUMN, so an unstaged gather of the HWC store would stride
// by a whole scene row.  One workgroup makes one 32 x 32 output tile of one kind of one sample, as K9 does for its
// rotated crops.  The tile's pre-image is a block of at most 32 x 32 source pixels (the frame maps move by at most one
// source index per frame index: border and extension only reflect); its rows are contiguous runs of at most 32 * 16 =
// 512 HWC bytes, read with coalesced dword loads into
//   lds[32][kPitch],  kPitch = 131 dwords (odd), 16.4 KiB: nine workgroups fit a CU's 160 KiB, the 32-wave cap admits eight.
// Bank arithmetic of the read-out: thread t owns output pixels (oy = t / 8, ox = 4 (t % 8) + p), p = 0..3; for one p the 32
// lanes that a 4-byte or 1-byte LDS read serves together hold 4 values of oy = 4 consecutive source COLUMNS and 8 values of
// ox = 8 source ROWS four apart.  Rows four apart are 4 * 131 = 524 = 12 (mod 32) banks apart: the eight rows start in
// banks 0, 12, 24, 4, 16, 28, 8, 20, all distinct and four apart (an even pitch would put them all into one bank: 8-way).
// The four columns add floor(col * pxb / 4) = 0..3 banks for the DEM (4 B a pixel) and the image (3 B): conflict-free; for
// a 15-channel mask (15 B a pixel: 0, 3, 7, 11) two of the 32 lanes can meet in a bank: 2-way at worst.  The writes are
// the 16-byte runs of the streaming kernel.  With frame maps that are not frame_maps' own a source pixel can lie outside
// the staged block: it is read from the store directly.  A window's block is its pre-image by construction.
#include "scene_prepare.h"

#include <cmath>

namespace {

using namespace jspsr;

// ---- the geometries ---------------------------------------------------------------------------------------------------
// kRow: int32 columns of a sample row {scene, base, ...}; the code, where one is read, is the last.
// quad: the source pixels of output pixels (Y, X .. X + 3), n of them inside the row -> okp, sy, sx.
// block / pixel (staged kernel): the pre-image block of output tile (Y0, X0) + th x tw, and the source pixel of tile
// pixel (oy, ox).

template <bool D4>
struct Frames {
  static constexpr int kRow = D4 ? 3 : 2;
  static constexpr bool kForeign = true;                     // the maps are the caller's: a pixel may miss the block
  using Coord = int;
  const int *ti, *tj;                                         // staged: transformed row / column of the tile's rows / columns

  static __device__ __forceinline__ void quad(const PrepareArgs& a, const int* row, bool ok, long long H, long long W, int Y,
                                              int X, int n, bool (&okp)[4], int (&sy)[4], int (&sx)[4]) {
    const int i = a.rows[Y];
    ok = ok && i >= 0 && i < H;
    for (int q = 0; q < 4; ++q) {
      const int j = a.cols[X + min(q, n - 1)];
      okp[q] = ok && j >= 0 && j < W;
      if (D4) {
        d4_source(row[2] & 15, (int)H, (int)W, i, j, sy[q], sx[q]);
      } else {
        sy[q] = i;
        sx[q] = j;
      }
    }
  }

  __device__ __forceinline__ Block block(const PrepareArgs& a, const int*, int code, long long H, long long W, int Y0, int X0,
                                         int th, int tw, int tid) {
    __shared__ int rows_t[kTile], cols_t[kTile];                      // -1 = none
    __shared__ int win[4];                                            // their ranges: i min, i max, j min, j max
    ti = rows_t;
    tj = cols_t;
    if (tid < 64) {                                                   // lanes 0..31 the tile's rows, 32..63 its columns
      const int t = tid & 31, isj = tid >> 5;
      int v = -1;
      if (t < (isj ? tw : th)) v = isj ? a.cols[X0 + t] : a.rows[Y0 + t];
      const bool in = v >= 0 && v < (isj ? H : W);                    // the transformed scene is W x H
      if (!in) v = -1;
      (isj ? cols_t : rows_t)[t] = v;
      int lo = in ? v : INT_MAX, hi = in ? v : INT_MIN;
      for (int m = 16; m; m >>= 1) {                                  // within each half of the wave
        lo = min(lo, __shfl_xor(lo, m));
        hi = max(hi, __shfl_xor(hi, m));
      }
      if (t == 0) { win[2 * isj] = lo; win[2 * isj + 1] = hi; }
    }
    __syncthreads();
    // the D4 map is axis-aligned and monotonic, so two opposite corners span the block
    Block k{0, 0, 0, 0};
    if (win[0] <= win[1] && win[2] <= win[3]) {
      int sy0, sx0, sy1, sx1;
      d4_source(code, (int)H, (int)W, win[0], win[2], sy0, sx0);
      d4_source(code, (int)H, (int)W, win[1], win[3], sy1, sx1);
      if (sy0 > sy1) { const int t = sy0; sy0 = sy1; sy1 = t; }
      if (sx0 > sx1) { const int t = sx0; sx0 = sx1; sx1 = t; }
      k = Block{sy0, sx0, min(sy1 - sy0 + 1, kTile), min(sx1 - sx0 + 1, kTile)};
    }
    return k;
  }

  __device__ __forceinline__ bool pixel(const PrepareArgs&, const int*, int code, long long H, long long W, int, int, int oy,
                                        int ox, int& py, int& px) const {
    const int i = ti[oy], j = tj[ox];
    if (i < 0 || j < 0) return false;
    d4_source(code, (int)H, (int)W, i, j, py, px);
    return true;
  }
};

template <bool D4>
struct Windows {
  static constexpr int kRow = D4 ? 5 : 4;
  static constexpr bool kForeign = false;
  using Coord = long long;                                    // y0 and x0 are the caller's

  static __device__ __forceinline__ void quad(const PrepareArgs& a, const int* row, bool ok, long long H, long long W, int Y,
                                              int X, int n, bool (&okp)[4], long long (&sy)[4], long long (&sx)[4]) {
    int wy = Y, wx = X, step = 1;                             // the first of the four in the window; the others lie in the
    if (D4) {                                                 // same window row, one column on or one column back
      const int code = row[4] & 11;                           // an even angle whatever the table holds
      d4_source(code, a.kh, a.kw, Y, X, wy, wx);
      step = ((code >> 3) ^ (code >> 1)) & 1 ? -1 : 1;        // a half turn or a mirror image, not both
    }
    const long long ay = (long long)row[2] + wy;
    ok = ok && ay >= 0 && ay < H;
    for (int q = 0; q < 4; ++q) {
      sy[q] = ay;
      sx[q] = (long long)row[3] + wx + step * (D4 ? min(q, n - 1) : q);
      okp[q] = ok && sx[q] >= 0 && sx[q] < W;
    }
  }

  // tw rows (an output column is a source row) by th columns of the window; then in the scene, clipped to it
  __device__ __forceinline__ Block block(const PrepareArgs& a, const int* row, int code, long long H, long long W, int Y0,
                                         int X0, int th, int tw, int) {
    int sya, sxa, syb, sxb;
    d4_source(code, a.kh, a.kw, Y0, X0, sya, sxa);
    d4_source(code, a.kh, a.kw, Y0 + th - 1, X0 + tw - 1, syb, sxb);
    const long long ay0 = (long long)row[2] + min(sya, syb), ax0 = (long long)row[3] + min(sxa, sxb);
    const long long cy0 = max(ay0, 0ll), cx0 = max(ax0, 0ll);
    return Block{cy0, cx0, (int)max(min(ay0 + tw, H) - cy0, 0ll), (int)max(min(ax0 + th, W) - cx0, 0ll)};   // <= 32 each
  }

  __device__ __forceinline__ bool pixel(const PrepareArgs& a, const int* row, int code, long long H, long long W, int Y0, int X0,
                                        int oy, int ox, int& py, int& px) const {
    int sy, sx;
    d4_source(code, a.kh, a.kw, Y0 + oy, X0 + ox, sy, sx);
    const long long ay = (long long)row[2] + sy, ax = (long long)row[3] + sx;
    if (!(ay >= 0 && ay < H && ax >= 0 && ax < W)) return false;
    py = (int)ay;
    px = (int)ax;
    return true;
  }
};

// ---- the kernels ------------------------------------------------------------------------------------------------------

template <template <bool> class Geometry, bool D4>
__global__ __launch_bounds__(256) void stream_kernel(PrepareArgs a) {
  using G = Geometry<D4>;
  const KindDesc& d = a.d[blockIdx.y];
  const int Wq = (a.Wp + 3) >> 2;                                     // quads of an output row
  const long long total = (long long)a.B * a.Hp * Wq;
  const int es = d.kind == LR_DEM ? 4 : 1;                            // bytes per channel value
  const int pxb = d.C * es;                                           // bytes per pixel
  const size_t plane = (size_t)a.Hp * a.Wp;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int X = (int)(idx % Wq) * 4;
    const long long r = idx / Wq;
    const int Y = (int)(r % a.Hp), b = (int)(r / a.Hp);
    const int n = min(4, a.Wp - X);
    const int* row = a.samples + (size_t)b * G::kRow;
    const float base = __int_as_float(row[1]);
    long long off, H, W;
    const bool ok = sample_scene<D4>(a, d, row[0], D4 ? row[G::kRow - 1] : 0, 0, pxb, off, H, W);
    typename G::Coord sy[4], sx[4];
    bool okp[4];
    G::quad(a, row, ok, H, W, Y, X, n, okp, sy, sx);
    const unsigned char* p[4];
    for (int q = 0; q < 4; ++q) p[q] = okp[q] && d.kind != COORD ? d.src + (off + sy[q] * W + sx[q]) * pxb : nullptr;
    float* o = d.out + ((size_t)b * d.cpitch + d.coff) * plane + (size_t)Y * a.Wp + X;
    write_quad<false>(a, d, o, plane, n, base, okp, sy, sx, H, W, [&](int q, int c) { return p[q] + c * es; });
  }
}

template <class G>
__global__ __launch_bounds__(256) void staged_kernel(PrepareArgs a, int tiles_x) {
  __shared__ unsigned int lds[kTile * kPitch];
  __shared__ int rowoff[kTile];                               // LDS byte offset of block row r's first pixel
  const KindDesc& d = a.d[blockIdx.z];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int Y0 = (blockIdx.x / tiles_x) * kTile, X0 = (blockIdx.x % tiles_x) * kTile;
  const int th = min(kTile, a.Hp - Y0), tw = min(kTile, a.Wp - X0);
  const int* row = a.samples + (size_t)b * G::kRow;
  const float base = __int_as_float(row[1]);
  const int code = (row[G::kRow - 1] & 15) | 4;                       // an odd angle whatever the table holds
  const int es = d.kind == LR_DEM ? 4 : 1;                            // bytes per channel value
  const int pxb = d.C * es;                                           // bytes per pixel
  long long off, H, W;
  const bool ok = sample_scene<true>(a, d, row[0], row[G::kRow - 1], 1, pxb, off, H, W);   // !ok: H = W = 0, an empty block
  G g;
  const Block k = g.block(a, row, code, H, W, Y0, X0, th, tw, tid);
  stage_block(d, k, off, W, pxb, tid, lds, rowoff);

  // thread tid owns output pixels (oy, ox .. ox + 3) of the tile in every channel: 32 rows x 8 groups of 4 = 256
  const int oy = tid >> 3, ox = (tid & 7) * 4;
  if (oy >= th || ox >= tw) return;
  const int n = min(4, tw - ox);
  const unsigned char* l8 = reinterpret_cast<const unsigned char*>(lds);
  int po[4], py[4], px[4];                                            // LDS byte offset (-1: not staged), scene row, column
  bool okp[4];
  for (int p = 0; p < 4; ++p) {
    py[p] = px[p] = 0;
    po[p] = -1;
    okp[p] = ok && g.pixel(a, row, code, H, W, Y0, X0, oy, ox + min(p, n - 1), py[p], px[p]);
    if (okp[p]) {
      const int r = py[p] - (int)k.y0, c = px[p] - (int)k.x0;           // okp: the block starts inside the scene
      if (!G::kForeign || (r >= 0 && r < k.nr && c >= 0 && c < k.nc)) po[p] = rowoff[r] + c * pxb;
    }
  }
  const size_t plane = (size_t)a.Hp * a.Wp;
  float* o = d.out + ((size_t)b * d.cpitch + d.coff) * plane + (size_t)(Y0 + oy) * a.Wp + X0 + ox;
  unsigned int raw[4];                                                // the channel's bytes, from the block or from the store
  write_quad<G::kForeign>(a, d, o, plane, n, base, okp, py, px, H, W, [&](int p, int c) {
    raw[p] = 0;
    if (d.kind != COORD) {
      if (!G::kForeign || po[p] >= 0) raw[p] = channel_bytes(l8 + po[p] + c * es, es);
      else raw[p] = channel_bytes(d.src + (off + (long long)py[p] * (int)W + px[p]) * pxb + c * es, es);   // W fits: a D4 scene
    }
    return reinterpret_cast<const unsigned char*>(&raw[p]);
  });
}

// ---- the entries ------------------------------------------------------------------------------------------------------

struct Entry {
  const char* name;           // for the messages
  bool frames;                // the geometry: frame maps (rows, cols), or a window per sample row
  const char* shares;         // with a D4 code: what the samples of a launch share, so hold one rot90 parity
};

// The checks of the four entries, in their order, and the kernels' argument block.  h, w: the frame's sides, or the
// upright window's.  codes: the host copy of the samples' codes, NULL for an upright entry.  -> 0 or the failure's code;
// odd: the launch's rot90 parity.
int pack(const Entry& e, PrepareArgs& a, int& nk, int& odd, const void* const* src, const long long* src_bytes, float* const* out,
         const int* channels, const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples,
         const int* codes, int B, const int* rows, const int* cols, int h, int w, int flags, double elev_min, double elev_max,
         int mask_div) {
  const bool d4 = e.shares != nullptr;
  if (!src || !src_bytes || !out || !channels || !coff || !cpitch || !scenes || !samples || (d4 && !codes) ||
      (e.frames && (!rows || !cols)) || n_scenes <= 0 || B <= 0 || (e.frames && d4 && B > 65535) || h <= 0 || w <= 0 ||
      !(elev_max > elev_min) || mask_div <= 0 || (flags & ~JSPSR_BATCH_FLAGS))
    return fail(JSPSR_EINVAL, "%s: bad arguments", e.name);
  if (d4 && B > 65535) return fail(JSPSR_EINVAL, "%s: %d samples, at most 65535 in a launch", e.name, B);
  if ((flags & JSPSR_BATCH_IMAGE_11) && (flags & JSPSR_BATCH_IMAGE_255))
    return fail(JSPSR_EINVAL, "%s: image range [-1, 1] and [0, 255] together", e.name);
  if (out[HR_DEM]) return fail(JSPSR_EINVAL, "%s: kind 1 (hr_dem) is not an input of the model", e.name);
  if (!e.frames && (!aligned4(samples) || (reinterpret_cast<uintptr_t>(scenes) & 7u)))
    return fail(JSPSR_EALIGN, "%s: tables not aligned to their element size", e.name);
  for (int b = 0; d4 && b < B; ++b) {
    if (codes[b] < 0 || codes[b] > 15) return fail(JSPSR_EINVAL, "%s: sample %d: code %d outside 0..15", e.name, b, codes[b]);
    if (((codes[b] ^ codes[0]) >> 2) & 1)
      return fail(JSPSR_EINVAL, "%s: sample %d: rot90 %d beside rot90 %d, a launch holds one parity (%s)", e.name, b,
                  codes[b] >> 2, codes[0] >> 2, e.shares);
  }
  odd = d4 ? (codes[0] >> 2) & 1 : 0;
  a = PrepareArgs{};
  a.kh = h;
  a.kw = w;
  a.Hp = !e.frames && odd ? w : h;                            // a quarter turn of a window transposes it; a frame is the
  a.Wp = !e.frames && odd ? h : w;                            // transformed scene's already
  nk = 0;
  for (int kind = 0; kind < kKinds; ++kind) {
    if (!out[kind]) continue;
    const int C = channels[kind];
    const int need = kind == COORD ? 2 : (kind == IMAGE || kind == MASK) ? -1 : 1;
    if (C <= 0 || C > kMaxC || (need > 0 && C != need) || coff[kind] < 0 || cpitch[kind] < coff[kind] + C)
      return fail(JSPSR_EINVAL, "%s: kind %d: bad channels (%d, offset %d, pitch %d)", e.name, kind, C, coff[kind], cpitch[kind]);
    if (!aligned4(out[kind])) return fail(JSPSR_EALIGN, "%s: kind %d: output not 4-byte aligned", e.name, kind);
    if (kind != COORD) {
      if (!src[kind] || src_bytes[kind] <= 0) return fail(JSPSR_EINVAL, "%s: kind %d: null or empty store", e.name, kind);
      if (!aligned4(src[kind])) return fail(JSPSR_EALIGN, "%s: kind %d: store not 4-byte aligned", e.name, kind);
    }
    a.d[nk++] = KindDesc{static_cast<const unsigned char*>(kind == COORD ? nullptr : src[kind]), kind == COORD ? 0 : src_bytes[kind],
                         out[kind], kind, C, coff[kind], cpitch[kind], (a.Wp & 3) == 0 && aligned16(out[kind])};
  }
  if (nk == 0) return fail(JSPSR_EINVAL, "%s: no output", e.name);
  a.scenes = scenes;
  a.samples = samples;
  a.rows = rows;
  a.cols = cols;
  a.n_scenes = n_scenes;
  a.B = B;
  a.flags = flags;
  a.mask_div = mask_div;
  a.lo = (float)elev_min;                                   // the Python numbers, as numpy casts them against fp32 arrays
  a.span = (float)(elev_max - elev_min);
  a.log_span = log(elev_max - elev_min);
  return 0;
}

template <template <bool> class Geometry, bool D4>
int launch(const Entry& e, const PrepareArgs& a, int nk, int odd, jspsr_stream_t stream) {
  if (odd) {
    const long long tiles_x = (a.Wp + kTile - 1) / kTile, tiles = tiles_x * ((a.Hp + kTile - 1) / kTile);
    if (tiles > INT_MAX)
      return fail(JSPSR_EINVAL, "%s: a %d x %d %s has too many tiles", e.name, a.kh, a.kw, e.frames ? "frame" : "window");
    hipLaunchKernelGGL(staged_kernel<Geometry<true>>, dim3((unsigned)tiles, a.B, nk), dim3(256), 0, static_cast<hipStream_t>(stream),
                       a, (int)tiles_x);
  } else {
    const long long items = (long long)a.B * a.Hp * ((a.Wp + 3) / 4);
    hipLaunchKernelGGL((stream_kernel<Geometry, D4>), dim3(blocks_for(items), nk), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  }
  return check_launch(e.name);
}

}  // namespace

extern "C" int jspsr_scene_prepare(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                                   const int* coff, const int* cpitch, const long long* scenes, int n_scenes, const int* samples,
                                   int B, const int* rows, const int* cols, int Hp, int Wp, int flags, double elev_min,
                                   double elev_max, int mask_div, jspsr_stream_t stream) {
  const Entry e{"scene_prepare", true, nullptr};
  PrepareArgs a;
  int nk, odd;
  const int rc = pack(e, a, nk, odd, src, src_bytes, out, channels, coff, cpitch, scenes, n_scenes, samples, nullptr, B, rows, cols,
                      Hp, Wp, flags, elev_min, elev_max, mask_div);
  return rc ? rc : launch<Frames, false>(e, a, nk, odd, stream);
}

extern "C" int jspsr_scene_prepare_d4(const void* const* src, const long long* src_bytes, float* const* out, const int* channels,
                                      const int* coff, const int* cpitch, const long long* scenes, int n_scenes,
                                      const int* samples, const int* codes, int B, const int* rows, const int* cols, int Hp,
                                      int Wp, int flags, double elev_min, double elev_max, int mask_div, jspsr_stream_t stream) {
  const Entry e{"scene_prepare_d4", true, "one frame"};
  PrepareArgs a;
  int nk, odd;
  const int rc = pack(e, a, nk, odd, src, src_bytes, out, channels, coff, cpitch, scenes, n_scenes, samples, codes, B, rows, cols,
                      Hp, Wp, flags, elev_min, elev_max, mask_div);
  return rc ? rc : launch<Frames, true>(e, a, nk, odd, stream);
}

extern "C" int jspsr_scene_prepare_windows(const void* const* src, const long long* src_bytes, float* const* out,
                                           const int* channels, const int* coff, const int* cpitch, const long long* scenes,
                                           int n_scenes, const int* samples, int B, int kh, int kw, int flags, double elev_min,
                                           double elev_max, int mask_div, jspsr_stream_t stream) {
  const Entry e{"scene_prepare_windows", false, nullptr};
  PrepareArgs a;
  int nk, odd;
  const int rc = pack(e, a, nk, odd, src, src_bytes, out, channels, coff, cpitch, scenes, n_scenes, samples, nullptr, B, nullptr,
                      nullptr, kh, kw, flags, elev_min, elev_max, mask_div);
  return rc ? rc : launch<Windows, false>(e, a, nk, odd, stream);
}

extern "C" int jspsr_scene_prepare_windows_d4(const void* const* src, const long long* src_bytes, float* const* out,
                                              const int* channels, const int* coff, const int* cpitch, const long long* scenes,
                                              int n_scenes, const int* samples, const int* codes, int B, int kh, int kw, int flags,
                                              double elev_min, double elev_max, int mask_div, jspsr_stream_t stream) {
  const Entry e{"scene_prepare_windows_d4", false, "one output shape"};
  PrepareArgs a;
  int nk, odd;
  const int rc = pack(e, a, nk, odd, src, src_bytes, out, channels, coff, cpitch, scenes, n_scenes, samples, codes, B, nullptr,
                      nullptr, kh, kw, flags, elev_min, elev_max, mask_div);
  return rc ? rc : launch<Windows, true>(e, a, nk, odd, stream);
}
