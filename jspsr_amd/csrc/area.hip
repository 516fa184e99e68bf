// K26 -- exact area downsample of HWC uint8 rasters on the device: image, mask and canopy held on a finer grid than their
// scene (0.5-2 m orthophotos and land cover under an 8 m target) are brought to the scene's grid here instead of by a host
// resize.  A LIST of rasters of different shapes and one channel count C <= 16 goes through ONE launch; every raster ratio
// >= 1 per axis, the extents taken as equal as K25 takes them.  Integers only where a value is decided.
//
// The rule, one axis: source length h, output length H, 1 <= H <= h.  In units where a source pixel has length H, output Y
// covers [Y h, (Y + 1) h) and source pixel i covers [i H, (i + 1) H); the weight is the overlap
//     a(Y, i) = min((Y + 1) h, (i + 1) H) - max(Y h, i H)          where positive          (area_weight below)
// so that sum_i a(Y, i) = h, sum_Y a(Y, i) = H, an output has taps i0 = floor(Y h / H) .. i1 = floor(((Y + 1) h - 1) / H), at
// most ceil(h / H) + 1 of them, and a source pixel lies under at most two outputs.  All products stay below 2^32 for sides
// up to 65535, which is what the entry accepts.  Per channel, with S = sum_y sum_x a_y a_x v and D = h w:
//     "area":      out = floor((S + floor(D / 2)) / D)              round half up, always 0 .. 255; H == h and W == w: the input
//     "majority":  (one-hot masks; a non-zero byte counts as 1) none = D - sum_c S_c, signed; c* the lowest index among the
//                  channels of largest S_c; the pixel is one-hot at c* iff S_c* > 0 and S_c* >= none, else all zeros.
// jspsr_area_axis gives first, count and the weights of an axis on the host from the same inline the kernel evaluates.
//
// Tiling.  The pass reads every source byte once and is bound by that read.  The unit of work is ONE WAVE: a band of 16
// output rows by TW = 64 output columns, a lane per column (all C channels of a pixel in one lane, as "majority" needs them).
// A workgroup is four such waves that share nothing -- no workgroup barrier, consecutive units lie side by side along x.
// The wave streams the source rows under its band top to bottom; the part of a source row under its 64 columns is ONE
// contiguous piece of HWC bytes, (64 ratio + 2) C at most.  It is read as the 16-byte blocks that cover it, from the 16-byte
// boundary below its first byte, each by one aligned 16-byte load of a lane, and written to the wave's own 4 KiB of LDS as
// it is.  C = 3 and odd pixel offsets start a piece anywhere in a block: the head is kept as a byte offset into the
// buffer, and a first or last block that is not wholly inside [src, src + bytes) is read byte by byte, its bytes outside
// never.  A step fills the four 16-byte registers of a lane: with the pieces of FOUR rows where a piece fits 64 blocks (1 KiB:
// ratios up to 5 at C = 3), a row per quarter of the buffer -- else with up to 4 KiB of whole pixels of one row, a chunk; a row
// is then as many chunks as it takes, so ratios of 16 and more (a 65535 -> 1 axis has 65535 taps) need no patch of the tile.
// The loads of the next step are issued before the taps of this one are summed.  A lane adds the taps of its column that
// lie in a chunk to its C horizontal sums hs_c = sum_x a_x v (< 2^24, 32 bit).  At the end of a source row sy the wave adds
// a_y(Y, sy) hs_c to its C 64-bit accumulators (the weight is the same for every lane: scalar); when (sy + 1) H >= (Y + 1) h the
// output row Y is complete, is written, and the row below starts from a_y(Y + 1, sy) hs_c -- the straddling row is not read
// again.  A source pixel that straddles two units is read by both; nothing else is read twice.  A lane past the raster's
// edge has no taps and helps with the loads.  Within a wave LDS operations complete in order, so the wave needs no barrier
// of its own either.  A wave walks its rows one after the other, each step a round trip to memory, so a call with few units
// (eight 334 x 334 scenes: 1008) would leave most of the chip idle: the entry halves the band, 16 -> 8 -> 4 -> 2 rows, while the
// call has fewer than 2048 units.  The arithmetic is exact, so the bytes do not depend on the band.
//
// The division by D (one per output byte, D the raster's constant, S + D / 2 < 2^40) is exact: q = trunc(double(S + D / 2) *
// (1.0 / double(D))) is within one of the quotient (both factors carry 53 bits, the quotient is at most 255), and the
// remainder S + D / 2 - q D, formed in integers, moves q down or up by one.  The reciprocal is formed once per wave.  Whatever
// rounding or contraction the estimate sees, the integer step decides the result, so the file needs no -ffp-contract entry.
// "majority" divides nothing.  No workspace, no host synchronisation, the same bits on every run and in any company.
#include "common.h"

#include <type_traits>

namespace {

using namespace jspsr;

constexpr int RB = 16, TW = 64;               // the output rows (at most) and columns of a wave's unit
constexpr int RB_MIN = 2;                     // the band of a call with few units
constexpr long long UNITS_MIN = 2048;         // 256 CUs x 8 waves
constexpr int WAVES = 4, NTHREADS = 64 * WAVES;
constexpr int CHUNK = 4096;                   // bytes of LDS per wave: the blocks of one chunk of a row piece
constexpr int BPL = CHUNK / (64 * 16);        // 16-byte blocks a lane loads per chunk
constexpr int ROW = 6;                        // table words per raster
constexpr long long SIDE_MAX = 65535;         // every product of the weights stays below 2^32

// The overlap of output Y (of H) with source pixel i (of h) in units of 1 / (h H) of the axis, 0 where they do not meet.
// Y < H <= h <= 65535 and i < h: no product passes 2^32.
// area_overlap takes the products: the output's extent [lo, hi) = [Y h, (Y + 1) h) and the pixel's start d = i H, which a loop
// over i steps by H.
__host__ __device__ __forceinline__ unsigned area_overlap(unsigned lo, unsigned hi, unsigned d, unsigned H) {
  const unsigned e = d + H, top = hi < e ? hi : e, bot = lo > d ? lo : d;
  return top > bot ? top - bot : 0u;
}
__host__ __device__ __forceinline__ unsigned area_weight(unsigned Y, unsigned i, unsigned h, unsigned H) {
  return area_overlap(Y * h, (Y + 1) * h, i * H, H);
}
__host__ __device__ __forceinline__ unsigned area_first(unsigned Y, unsigned h, unsigned H) { return Y * h / H; }
__host__ __device__ __forceinline__ unsigned area_last(unsigned Y, unsigned h, unsigned H) { return ((Y + 1) * h - 1) / H; }

// One 16-byte block at the 16-byte aligned address src + off (off may lie up to 15 bytes below 0); a block that is not wholly
// inside [src, src + bytes) byte by byte, the bytes outside left unread (zero).  Addressed from the kernel's own pointer, so
// that the loads are global ones, which need not wait for the LDS traffic around them.
__device__ __forceinline__ uint4 load_block(const unsigned char* __restrict__ src, long long off, long long bytes) {
  if (off >= 0 && off + 16 <= bytes) return *reinterpret_cast<const uint4*>(src + off);
  unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
  for (int q = 0; q < 4; ++q)
#pragma unroll 1
    for (int b = 0; b < 4; ++b) {
      const long long o = off + 4 * q + b;
      if (o >= 0 && o < bytes) v[q] |= (unsigned)src[o] << (8 * b);
    }
  return make_uint4(v[0], v[1], v[2], v[3]);
}

struct Chunk {                                // chunk k of the piece of source row sy, the same for every lane of the wave
  unsigned p0, npx, head, nblk;               // first source column, columns, the first byte's offset in its block, blocks
  long long ga;                               // the first block's offset from src in bytes, a multiple of 16 from the address
};

template <int C>
__device__ __forceinline__ Chunk chunk_of(const unsigned char* src, long long src_off, unsigned w, unsigned sx0, unsigned sx1,
                                          unsigned sy, unsigned k) {
  constexpr unsigned PPC = (CHUNK - 16) / C;  // whole pixels of a chunk, room for the head left
  Chunk c;
  c.p0 = sx0 + k * PPC;
  c.npx = sx1 + 1 - c.p0 < PPC ? sx1 + 1 - c.p0 : PPC;
  const long long gs = (src_off + (long long)sy * w + c.p0) * C;              // the first byte's offset from src
  c.head = (unsigned)((reinterpret_cast<uintptr_t>(src) + (unsigned long long)gs) & 15u);
  c.ga = gs - c.head;
  c.nblk = (c.head + c.npx * C + 15) >> 4;    // <= CHUNK / 16
  return c;
}

// The pass lives on loads in flight: few channels leave room for five waves per SIMD, and the registers are held to that.
template <int C, bool MAJ>
__global__ __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(C <= 4 ? 5 : (C <= 8 ? 4 : 2))))
void area_kernel(const unsigned char* __restrict__ src, long long src_bytes, const long long* __restrict__ table,
                 unsigned char* __restrict__ dst, int words, int rb) {
  constexpr unsigned PPC = (CHUNK - 16) / C;
  __shared__ uint4 stage[WAVES][CHUNK / 16];
  const long long* __restrict__ row = table + (size_t)blockIdx.y * ROW;
  const long long src_off = row[0], dst_off = row[3];
  const unsigned h = (unsigned)row[1], w = (unsigned)row[2], H = (unsigned)row[4], W = (unsigned)row[5];
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const unsigned xtiles = (W + TW - 1) / TW, bands = (H + rb - 1) / rb;
  const unsigned long long unit = (unsigned long long)blockIdx.x * WAVES + wave;
  if (unit >= (unsigned long long)xtiles * bands) return;        // wave-uniform, and no workgroup barrier anywhere
  const unsigned Yb = (unsigned)(unit / xtiles) * rb, X0 = (unsigned)(unit % xtiles) * TW;
  const unsigned Ye = Yb + rb < H ? Yb + rb : H, tw = W - X0 < TW ? W - X0 : TW;
  const bool live = (unsigned)lane < tw;
  const unsigned X = X0 + lane;
  unsigned i0 = 1, i1 = 0;                                       // a lane past the edge: no taps
  if (live) {
    i0 = area_first(X, w, W);
    i1 = area_last(X, w, W);
  }
  const unsigned sx0 = area_first(X0, w, W), sx1 = area_last(X0 + tw - 1, w, W);
  const unsigned sy0 = area_first(Yb, h, H), sy1 = area_last(Ye - 1, h, H);
  const unsigned nchunks = (sx1 - sx0 + PPC) / PPC;
  // a piece of at most 64 blocks: a step takes BPL rows, a row per quarter of the buffer; else one row, BPL x 64 blocks of it
  const bool rows = (sx1 - sx0 + 1) * C + 15 <= 64 * 16;
  const unsigned R = rows ? BPL : 1;
  uint4* buf = stage[wave];                                      // written as blocks, read as bytes: the same memory
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(buf);
  const unsigned long long D = (unsigned long long)h * w;
  const double rD = 1.0 / (double)D;

  using acc_t = typename std::conditional<MAJ, unsigned, unsigned long long>::type;       // a coverage S_c is at most D < 2^32
  acc_t acc[C];
  unsigned hs[C];
  const unsigned xlo = X * w, xhi = xlo + w;                     // the column's extent in units of 1 / (w W)
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0;
  unsigned Y = Yb;
  uint4 r[BPL];
  // the loads of step (sy, k): slot j is block lane + 64 j of the chunk, or block lane of row sy + j.  A lane past the last
  // block (or a slot past the last row) loads the last one again, so that nothing in the common path is conditional and
  // the loads stay in flight; only a step that touches the first or the last 16 bytes of src takes the careful loads.
  auto issue = [&](unsigned sy, unsigned k) __attribute__((always_inline)) {
    long long off[BPL];
    bool edge = false;                                           // the same for the whole wave
#pragma unroll
    for (int j = 0; j < BPL; ++j) {
      const unsigned y = rows ? (sy + j < sy1 ? sy + j : sy1) : sy, blk = rows ? (unsigned)lane : (unsigned)lane + 64 * j;
      const Chunk c = chunk_of<C>(src, src_off, w, sx0, sx1, y, k);
      off[j] = c.ga + 16ll * (blk < c.nblk ? blk : c.nblk - 1);
      edge |= c.ga < 0 || c.ga + 16ll * c.nblk > src_bytes;
    }
    if (!edge) {
#pragma unroll
      for (int j = 0; j < BPL; ++j) r[j] = *reinterpret_cast<const uint4*>(src + off[j]);
    } else {
#pragma unroll
      for (int j = 0; j < BPL; ++j) r[j] = load_block(src, off[j], src_bytes);
    }
  };
  // the end of source row sy: its horizontal sums go to the accumulators, and a completed output row is written
  auto finish = [&](unsigned sy) __attribute__((always_inline)) {
    const unsigned ay = area_weight(Y, sy, h, H);
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += (acc_t)ay * hs[c];
    while (Y < Ye && (sy + 1) * H >= (Y + 1) * h) {              // sy is the last source row of output row Y
      unsigned char out[C];
      if (MAJ) {
        acc_t best = acc[0];
        long long sum = 0;
        int cb = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          sum += (long long)acc[c];
          if (acc[c] > best) {
            best = acc[c];
            cb = c;
          }
        }
        const bool hot = best > 0 && (long long)best >= (long long)D - sum;
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = hot && c == cb ? 1 : 0;
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const unsigned long long n = acc[c] + (D >> 1);
          unsigned q = (unsigned)((double)n * rD);
          const long long rem = (long long)(n - (unsigned long long)q * D);
          if (rem < 0) --q;
          else if (rem >= (long long)D) ++q;
          out[c] = (unsigned char)q;
        }
      }
      if (live) {
        unsigned char* __restrict__ o = dst + (dst_off + (long long)Y * W + X) * C;
        if (C % 4 == 0 && words) {
#pragma unroll
          for (int c4 = 0; c4 < C / 4; ++c4)
            reinterpret_cast<unsigned*>(o)[c4] = (unsigned)out[4 * c4] | (unsigned)out[4 * c4 + 1] << 8 | (unsigned)out[4 * c4 + 2] << 16 |
                                                 (unsigned)out[4 * c4 + 3] << 24;
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) o[c] = out[c];
        }
      }
      ++Y;
      const unsigned a2 = Y < Ye ? area_weight(Y, sy, h, H) : 0u;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = (acc_t)a2 * hs[c];
    }
  };
  issue(sy0, 0);
  for (unsigned sy = sy0; sy <= sy1; sy += R) {
    for (unsigned k = 0; k < nchunks; ++k) {
#pragma unroll
      for (int j = 0; j < BPL; ++j)
        buf[lane + 64 * j] = r[j];                               // blocks past the step's last one land in unused LDS
      const bool wrap = k + 1 == nchunks;
      if (!wrap || sy + R <= sy1) issue(wrap ? sy + R : sy, wrap ? 0 : k + 1);     // the next step's loads fly while this one is summed
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (unsigned jr = 0; jr < R && sy + jr <= sy1; ++jr) {
        const unsigned y = sy + jr;
        const Chunk now = chunk_of<C>(src, src_off, w, sx0, sx1, y, k);
        if (k == 0) {
#pragma unroll
          for (int c = 0; c < C; ++c) hs[c] = 0;
        }
        const unsigned pe = now.p0 + now.npx - 1;
        const unsigned lo = i0 > now.p0 ? i0 : now.p0, hi = i1 < pe ? i1 : pe;
        unsigned d = lo * W, o = jr * (64 * 16) + now.head + (lo - now.p0) * C;
        for (unsigned i = lo; i <= hi; ++i, d += W, o += C) {
          const unsigned a = area_overlap(xlo, xhi, d, W);       // at most W < 2^16, a byte beside it: 24-bit products
          if (C % 4 == 0 && words) {                             // the pixel starts on a dword
#pragma unroll
            for (int c4 = 0; c4 < C / 4; ++c4) {
              const unsigned v4 = *reinterpret_cast<const unsigned*>(bytes + o + 4 * c4);
#pragma unroll
              for (int b = 0; b < 4; ++b) {
                unsigned v = (v4 >> (8 * b)) & 255u;
                if (MAJ) v = v != 0;
                hs[4 * c4 + b] += __umul24(a, v);
              }
            }
          } else {
#pragma unroll
            for (int c = 0; c < C; ++c) {
              unsigned v = bytes[o + c];
              if (MAJ) v = v != 0;
              hs[c] += __umul24(a, v);
            }
          }
        }
        if (k + 1 == nchunks) finish(y);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();                           // the next step is written over this one
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

template <int C>
void launch(bool maj, dim3 grid, hipStream_t s, const unsigned char* src, long long src_bytes, const long long* table,
            unsigned char* dst, int words, int rb) {
  if (maj) hipLaunchKernelGGL((area_kernel<C, true>), grid, dim3(NTHREADS), 0, s, src, src_bytes, table, dst, words, rb);
  else hipLaunchKernelGGL((area_kernel<C, false>), grid, dim3(NTHREADS), 0, s, src, src_bytes, table, dst, words, rb);
}

}  // namespace

extern "C" int jspsr_area_axis(int h, int H, int* first, int* count, unsigned* weights) {
  if (!first || !count) return fail(JSPSR_EINVAL, "area_axis: null pointer");
  if (h < 1 || H < 1 || H > h || h > SIDE_MAX)
    return fail(JSPSR_EINVAL, "area_axis: %d -> %d (1 <= H <= h <= %lld: a downsampling or the identity, upsampling is not built)", h, H,
                SIDE_MAX);
  const int taps = (h + H - 1) / H + 1;
  for (int Y = 0; Y < H; ++Y) {
    const unsigned i0 = area_first(Y, h, H), i1 = area_last(Y, h, H);
    first[Y] = (int)i0;
    count[Y] = (int)(i1 - i0 + 1);
    if (!weights) continue;
    for (int k = 0; k < taps; ++k) weights[(size_t)Y * taps + k] = i0 + k <= i1 ? area_weight(Y, i0 + k, h, H) : 0u;
  }
  return JSPSR_OK;
}

extern "C" int jspsr_area_forward(const unsigned char* src, long long src_numel, unsigned char* dst, long long dst_numel,
                                  const long long* table, const long long* host_table, int n, int channels, int mode,
                                  jspsr_stream_t stream) {
  const char* const name = "area_forward";
  if (!src || !dst || !table || !host_table) return fail(JSPSR_EINVAL, "%s: null pointer", name);
  if (mode != JSPSR_AREA_MEAN && mode != JSPSR_AREA_MAJORITY) return fail(JSPSR_EINVAL, "%s: mode %d", name, mode);
  if (channels < 1 || channels > 16) return fail(JSPSR_EINVAL, "%s: %d channels, the kernel takes 1..16", name, channels);
  if (n < 1 || n > 65535) return fail(JSPSR_EINVAL, "%s: %d rasters, one call takes 1..65535", name, n);
  if (src_numel < 0 || dst_numel < 0 || src_numel > (1ll << 58) || dst_numel > (1ll << 58))
    return fail(JSPSR_EINVAL, "%s: %lld source and %lld destination pixels", name, src_numel, dst_numel);
  if (reinterpret_cast<uintptr_t>(table) & 7u) return fail(JSPSR_EALIGN, "%s: table not 8-byte aligned", name);
  long long max_blocks = 0;
  for (int k = 0; k < n; ++k) {                                  // every index the kernel forms stays inside the buffers
    const long long* r = host_table + (size_t)k * ROW;
    const long long so = r[0], h = r[1], w = r[2], dof = r[3], H = r[4], W = r[5];
    if (h < 1 || w < 1 || H < 1 || W < 1)
      return fail(JSPSR_EINVAL, "%s: raster %d is %lld x %lld -> %lld x %lld: an empty side", name, k, h, w, H, W);
    if (H > h || W > w)
      return fail(JSPSR_EINVAL, "%s: raster %d is %lld x %lld -> %lld x %lld: upsampling is not built", name, k, h, w, H, W);
    if (h > SIDE_MAX || w > SIDE_MAX)                            // weights and their products in 32 bits, S + D / 2 < 2^40
      return fail(JSPSR_EINVAL, "%s: raster %d is %lld x %lld: a side above %lld does not fit the 32-bit weight arithmetic", name, k,
                  h, w, SIDE_MAX);
    if (so < 0 || h * w > src_numel - so || dof < 0 || H * W > dst_numel - dof)
      return fail(JSPSR_EINVAL, "%s: raster %d leaves its buffer (source %lld + %lld of %lld, destination %lld + %lld of %lld)", name, k,
                  so, h * w, src_numel, dof, H * W, dst_numel);
  }
  // the band of a unit: RB rows, halved while the call has too few units to fill the chip (a unit is one wave, and a wave
  // walks its rows one after the other); the arithmetic is exact, so the bytes do not depend on it
  auto units = [&](int k, int rb) {
    const long long* r = host_table + (size_t)k * ROW;
    return ((r[4] + rb - 1) / rb) * ((r[5] + TW - 1) / TW);
  };
  int rb = RB;
  for (; rb > RB_MIN; rb >>= 1) {
    long long total = 0;
    for (int k = 0; k < n && total < UNITS_MIN; ++k) total += units(k, rb);
    if (total >= UNITS_MIN) break;
  }
  for (int k = 0; k < n; ++k) {
    const long long blocks = (units(k, rb) + WAVES - 1) / WAVES;
    max_blocks = blocks > max_blocks ? blocks : max_blocks;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)max_blocks, (unsigned)n);            // at most 32768 * 1024 / 4 blocks of a raster
  const int words = channels % 4 == 0 && aligned4(src) && aligned4(dst);
  const bool maj = mode == JSPSR_AREA_MAJORITY;
  const long long src_bytes = src_numel * channels;
  switch (channels) {
#define JSPSR_AREA_CASE(C) case C: launch<C>(maj, grid, s, src, src_bytes, table, dst, words, rb); break;
    JSPSR_AREA_CASE(1) JSPSR_AREA_CASE(2) JSPSR_AREA_CASE(3) JSPSR_AREA_CASE(4) JSPSR_AREA_CASE(5) JSPSR_AREA_CASE(6)
    JSPSR_AREA_CASE(7) JSPSR_AREA_CASE(8) JSPSR_AREA_CASE(9) JSPSR_AREA_CASE(10) JSPSR_AREA_CASE(11) JSPSR_AREA_CASE(12)
    JSPSR_AREA_CASE(13) JSPSR_AREA_CASE(14) JSPSR_AREA_CASE(15) JSPSR_AREA_CASE(16)
#undef JSPSR_AREA_CASE
  }
  return check_launch(maj ? "area (majority)" : "area");
}
