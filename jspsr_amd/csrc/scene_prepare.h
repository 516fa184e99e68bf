// The parts that the whole-scene prepare entries share (K13-K16: scene_prepare.hip; the steps after the model are in
// scene_finish.h).
//
// prepare: out[b][c][Y][X] = ToTensor_kind(store pixel (sy, sx) of sample b's scene), (sy, sx) = geometry(b, Y, X).  The
// geometry is a compile-time policy of the two kernel templates in scene_prepare.hip; everything here is the same for
// every geometry: the argument block, the scene lookup, the staging of a block of the HWC store in LDS and its read-out,
// and the epilogue that writes four consecutive pixels of a row in every channel of a kind.
// Every translation unit that includes this is built with -ffp-contract=off (csrc/Makefile).
#pragma once
#include "common.h"
#include "d4.h"
#include "scene_finish.h"   // store_quad
#include "totensor.h"

#include <climits>

namespace jspsr {

constexpr int kTile = 32;                                   // output tile side of the staged kernels (and of finish_mean)
constexpr int kPitch = (kTile * kMaxC + 8) / 4 | 1;        // LDS row pitch in dwords: 32 px x 16 B + the unaligned head, odd

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
  const int* samples;         // [B][n] {scene, base (fp32 bits), the geometry's columns} (scene_prepare.hip)
  const int* rows;            // frame maps: [Hp] row of the (transformed) scene at output row Y, [Wp] column at output
  const int* cols;            //   column X; NULL for windows
  int n_scenes, B;
  int Hp, Wp;                 // the output plane: the frame, or the (transformed) window
  int kh, kw;                 // the sides as the caller gave them: the frame's, or the upright window's
  int flags, mask_div;
  float lo, span;             // fp32(elev_min), fp32(elev_max - elev_min)
  double log_span;            // log(elev_max - elev_min)
};

// The scene `scene` of the table: false unless it lies inside the store of kind d.  With a D4 code the sides must fit an
// int and the code must have the launch's rot90 parity.
template <bool D4>
__device__ __forceinline__ bool sample_scene(const PrepareArgs& a, const KindDesc& d, int scene, int code, int parity, int pxb,
                                             long long& off, long long& H, long long& W) {
  off = 0; H = 0; W = 0;
  if (scene < 0 || scene >= a.n_scenes) return false;
  if (D4 && (code < 0 || code > 15 || ((code >> 2) & 1) != parity)) return false;
  const long long o = a.scenes[scene * 3], h = a.scenes[scene * 3 + 1], w = a.scenes[scene * 3 + 2];
  if (o < 0 || h <= 0 || w <= 0 || (D4 && (h > INT_MAX || w > INT_MAX))) return false;
  if (d.kind == COORD ? !(h > 1 && w > 1) : (o + h * w) * pxb > d.src_bytes) return false;
  off = o; H = h; W = w;
  return true;
}

// Four consecutive pixels of an output row (n of them inside it) in every channel of the kind: pixel q is ToTensor of
// the bytes at bytes(q, c), source pixel (sy[q], sx[q]) of its H x W scene, or NaN where !okp[q].  Rolled: the loop over the
// four stays a loop -- for a reader with a second source (the staged kernel's read from the store), whose four addresses
// would otherwise be kept across the channels: 44 VGPRs against 38.
template <bool Rolled, class Coord, class Bytes>
__device__ __forceinline__ void write_quad(const PrepareArgs& a, const KindDesc& d, float* o, size_t plane, int n, float base,
                                           const bool (&okp)[4], const Coord (&sy)[4], const Coord (&sx)[4], long long H,
                                           long long W, Bytes&& bytes) {
  constexpr int kUnroll = Rolled ? 1 : 4;
  for (int c = 0; c < d.C; ++c, o += plane) {
    float v[4];
#pragma unroll kUnroll
    for (int q = 0; q < 4; ++q)
      v[q] = okp[q] ? transform(d.kind, c, bytes(q, c), base, (int)sy[q], (int)sx[q], H, W, a) : __int_as_float(0x7fc00000);
    store_quad(o, v, n, d.vec);
  }
}

// A block of nr <= 32 rows by nc <= 32 columns of a scene, from pixel (y0, x0)
struct Block {
  long long y0, x0;
  int nr, nc;
};

// Stage the block's HWC bytes: row r = scene bytes [s, s + nc * pxb), at most 512, read as the aligned dwords that cover
// it (128 + 2 at most) into lds[r][kPitch]; rowoff[r] = the LDS byte offset of its first pixel.  Bytes past the end of the
// store are never touched: a dword that straddles it is read byte by byte.  Ends with a barrier.
__device__ __forceinline__ void stage_block(const KindDesc& d, const Block& k, long long off, long long W, int pxb, int tid,
                                            unsigned int* lds, int* rowoff) {
  const int seg = k.nc * pxb;
  if (tid < k.nr) rowoff[tid] = tid * kPitch * 4 + (int)((off + (k.y0 + tid) * W + k.x0) * pxb & 3);
  if (d.kind != COORD && k.nc > 0) {
    const int ndw = seg / 4 + 2;                                      // <= kPitch
    for (int idx = tid; idx < k.nr * ndw; idx += 256) {
      const int r = idx / ndw, j = idx - r * ndw;
      const long long s = (off + (k.y0 + r) * W + k.x0) * pxb;
      const long long a0 = (s & ~3ll) + 4ll * j;
      if (a0 >= s + seg) continue;
      unsigned int v;
      if (a0 + 4 <= d.src_bytes) {
        v = *reinterpret_cast<const unsigned int*>(d.src + a0);
      } else {
        v = 0;
        for (int q = 0; q < 4; ++q)
          if (a0 + q < d.src_bytes) v |= (unsigned int)d.src[a0 + q] << (8 * q);
      }
      lds[r * kPitch + j] = v;
    }
  }
  __syncthreads();
}

// One channel value's bytes, es = 4 or 1 of them
__device__ __forceinline__ unsigned int channel_bytes(const unsigned char* p, int es) {
  return es == 4 ? *reinterpret_cast<const unsigned int*>(p) : (unsigned int)*p;
}

}  // namespace jspsr
