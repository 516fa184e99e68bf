// K17 -- voids in whole-scene inference: an exact nearest-seed transform over all scenes of a store, the fill and the
// output mask that use it.
//   jspsr_scene_nearest_seed   per pixel the nearest seed pixel of the same scene (index and squared distance), exact
//   jspsr_scene_fill_voids     lr_dem[void] = lr_dem[nearest valid pixel] (or the scene's base), in place
//   jspsr_scene_mask_out       result[void_out] = the no-data value, every scene of a predict_scenes call in one launch
// What they replace is a Euclidean feature transform and a gather on the host, a second upload of the store and a
// numpy np.where over the results.
//
// The rule (include/jspsr_hip.h): the seed that minimises (dy^2 + dx^2, |dx|, dx, dy) lexicographically.
// It is what the two-phase scheme below produces, and the scheme is all integer: every run gives the same bits.
//
// Phase 1, per column: dy to the nearest seed of the column, ties to the upper one, as int16 (2 B per pixel of workspace).
//   A column is cut into bands of 64 rows so that a tall, narrow scene still fills the chip (one thread per column would
//   be W threads): a thread owns (band, column), consecutive lanes consecutive columns, so every load and store of a wave
//   is one run of a row.  band_summary_kernel writes the first and the last seed row of every (band, column) -- into the
//   band's first row of the src and d2 planes, which phase 2 overwrites later: no further workspace and no per-scene
//   offsets beyond the pixel offset.  column_distance_kernel gathers its band's 64 seed bytes into a 64-bit mask, finds the
//   nearest seed row above and below the band by walking the summaries (one read per band passed; with a limit no further
//   than the limit reaches) and writes the 64 distances from the mask with clz / ctz.
// Phase 2, per row: a workgroup stages the row's int16 column distances in LDS (a 32767-wide row is 64 KB) and every thread
//   walks outwards from its pixel, x, x-1, x+1, x-2, ..., over k^2 + g^2, strict improvements only, until k^2 >= best or
//   k > limit or both sides have left the row.  Cost: O(distance to the nearest seed) LDS reads per query; a seed pixel
//   ends at k = 1; the lanes of a wave run to the longest search among them.  Wide seedless regions are where it degrades
//   (a lower-envelope phase 2 is the remedy).
//
// Every scene is checked on the device against the plane's length before a pixel of it is touched (a scene that does not
// fit is skipped), so no table can send an access outside the planes.  No float arithmetic, no atomics, no inline asm.
#include "common.h"

#include <climits>

namespace {

using namespace jspsr;

constexpr int kMaxSide = 32767;          // d2 < 2^31, dy fits int16
constexpr int kBand = 64;                // rows per band: one 64-bit mask per (band, column)
constexpr int kNone = -32768;            // int16: no seed in this column (within reach)
constexpr int kMaxGridX = 32768;

__device__ __forceinline__ bool scene_geom(const long long* __restrict__ t, int s, long long total, long long& off, int& H,
                                           int& W) {
  off = t[3 * s];
  const long long h = t[3 * s + 1], w = t[3 * s + 2];
  if (off < 0 || h <= 0 || w <= 0 || h > kMaxSide || w > kMaxSide || off > total || h * w > total - off) return false;
  H = (int)h;
  W = (int)w;
  return true;
}

// first[q], last[q], q = the pixel (band * 64, x): the first and the last seed row of the band in column x, or -1
__global__ __launch_bounds__(256) void band_summary_kernel(const unsigned char* __restrict__ seed,
                                                           const long long* __restrict__ scenes, int n, long long total,
                                                           int* __restrict__ first, int* __restrict__ last) {
  for (int s = blockIdx.y; s < n; s += gridDim.y) {
    long long off;
    int H, W;
    if (!scene_geom(scenes, s, total, off, H, W)) continue;
    const int nb = (H + kBand - 1) / kBand;
    const long long items = (long long)nb * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
      const int band = (int)(i / W), x = (int)(i - (long long)band * W);
      const int y0 = band * kBand, rows = min(kBand, H - y0);
      const long long q = off + (long long)y0 * W + x;
      const unsigned char* p = seed + q;
      int f = -1, l = -1;
      for (int r = 0; r < rows; ++r) {
        if (p[(long long)r * W]) {
          f = f < 0 ? y0 + r : f;
          l = y0 + r;
        }
      }
      first[q] = f;
      last[q] = l;
    }
  }
}

// g[p] = (row of the nearest seed of p's column) - (row of p), ties to the upper seed; kNone without one
__global__ __launch_bounds__(256) void column_distance_kernel(const unsigned char* __restrict__ seed,
                                                              const long long* __restrict__ scenes, int n, long long total,
                                                              int limit, const int* __restrict__ first,
                                                              const int* __restrict__ last, short* __restrict__ g) {
  for (int s = blockIdx.y; s < n; s += gridDim.y) {
    long long off;
    int H, W;
    if (!scene_geom(scenes, s, total, off, H, W)) continue;
    const int nb = (H + kBand - 1) / kBand;
    // a seed c + 1 bands away is at least 64 c + 1 rows away: past the limit it cannot be within it
    const int reach = limit > 0 ? min(nb, (limit + kBand - 1) / kBand + 1) : nb;
    const long long items = (long long)nb * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
      const int band = (int)(i / W), x = (int)(i - (long long)band * W);
      const int y0 = band * kBand, rows = min(kBand, H - y0);
      const long long q = off + (long long)y0 * W + x;
      const unsigned char* p = seed + q;
      unsigned long long mask = 0;
      for (int r = 0; r < rows; ++r) mask |= (unsigned long long)(p[(long long)r * W] != 0) << r;
      int up = -1, dn = -1;
      for (int b = band - 1, c = 0; b >= 0 && c < reach; --b, ++c) {
        const int r = last[off + (long long)b * kBand * W + x];
        if (r >= 0) { up = r; break; }
      }
      for (int b = band + 1, c = 0; b < nb && c < reach; ++b, ++c) {
        const int r = first[off + (long long)b * kBand * W + x];
        if (r >= 0) { dn = r; break; }
      }
      short* o = g + q;
      for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        const unsigned long long le = mask & (~0ull >> (63 - r)), ge = mask & (~0ull << r);
        const int ya = le ? y0 + 63 - __clzll((long long)le) : up;
        const int yb = ge ? y0 + __ffsll((long long)ge) - 1 : dn;
        const int da = ya >= 0 ? y - ya : INT_MAX, db = yb >= 0 ? yb - y : INT_MAX;
        int dy = kNone;
        if (da != INT_MAX || db != INT_MAX) dy = da <= db ? -da : db;
        o[(long long)r * W] = (short)dy;
      }
    }
  }
}

__global__ __launch_bounds__(256) void row_search_kernel(const short* __restrict__ g, const long long* __restrict__ scenes,
                                                         int n, long long total, int limit, int* __restrict__ src,
                                                         int* __restrict__ d2) {
  extern __shared__ short row[];                                      // the row's column distances, W of them
  const int lim2 = limit > 0 ? limit * limit : INT_MAX;               // limit <= 46340 (the entry maps larger ones to none)
  for (int s = blockIdx.y; s < n; s += gridDim.y) {
    long long off;
    int H, W;
    if (!scene_geom(scenes, s, total, off, H, W)) continue;           // the same for every thread of the workgroup
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
      const long long p0 = off + (long long)y * W;
      __syncthreads();                                                // the previous row's searches are over
      for (int x = threadIdx.x; x < W; x += 256) row[x] = g[p0 + x];
      __syncthreads();
      for (int x = threadIdx.x; x < W; x += 256) {
        int best = INT_MAX, bx = -1;
        const int g0 = row[x];
        if (g0 != kNone) { best = g0 * g0; bx = x; }
        int kmax = max(x, W - 1 - x);
        if (limit > 0) kmax = min(kmax, limit);
        for (int k = 1; k <= kmax && k * k < best; ++k) {
          const int k2 = k * k;
          if (x - k >= 0) {
            const int t = row[x - k];
            if (t != kNone && k2 + t * t < best) { best = k2 + t * t; bx = x - k; }
          }
          if (x + k < W) {
            const int t = row[x + k];
            if (t != kNone && k2 + t * t < best) { best = k2 + t * t; bx = x + k; }
          }
        }
        const bool found = bx >= 0 && best <= lim2;
        src[p0 + x] = found ? (y + row[bx]) * W + bx : -1;
        d2[p0 + x] = found ? best : -1;
      }
    }
  }
}

__global__ __launch_bounds__(256) void fill_voids_kernel(float* __restrict__ dem, const unsigned char* __restrict__ voids,
                                                         const int* __restrict__ src, const long long* __restrict__ scenes,
                                                         const float* __restrict__ base, int n, long long total) {
  for (int s = blockIdx.y; s < n; s += gridDim.y) {
    long long off;
    int H, W;
    if (!scene_geom(scenes, s, total, off, H, W)) continue;
    const long long px = (long long)H * W;
    const float b = base[s];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < px; i += (long long)gridDim.x * 256) {
      const long long p = off + i;
      if (!voids[p]) continue;
      const int t = src ? src[p] : -1;
      // a source is a valid pixel of the same scene: such a value is never written, so no value is both read and written
      dem[p] = (t >= 0 && t < px && !voids[off + t]) ? dem[off + t] : b;
    }
  }
}

__global__ __launch_bounds__(256) void mask_out_kernel(float* __restrict__ out, long long out_len,
                                                       const unsigned char* __restrict__ void_out, long long total,
                                                       const long long* __restrict__ rows, int m, float nodata) {
  for (int r = blockIdx.y; r < m; r += gridDim.y) {
    const long long ro = rows[3 * r], so = rows[3 * r + 1], px = rows[3 * r + 2];
    if (ro < 0 || so < 0 || px <= 0 || ro > out_len || px > out_len - ro || so > total || px > total - so) continue;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < px; i += (long long)gridDim.x * 256)
      if (void_out[so + i]) out[ro + i] = nodata;
  }
}

int grid_x(long long items) {
  long long b = (items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > kMaxGridX ? kMaxGridX : b));
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" size_t jspsr_scene_nearest_seed_workspace_bytes(long long pixels) {
  return pixels <= 0 ? 0 : ((size_t)pixels * sizeof(short) + 15) / 16 * 16;
}

extern "C" int jspsr_scene_nearest_seed(const unsigned char* seed, long long pixels, const long long* scenes,
                                        const long long* scenes_host, int n_scenes, int limit, int* src, int* d2,
                                        void* workspace, jspsr_stream_t stream) {
  if (!seed || !scenes || !scenes_host || !src || !d2 || !workspace || pixels <= 0 || n_scenes <= 0)
    return jspsr::fail(JSPSR_EINVAL, "scene_nearest_seed: bad arguments");
  if (limit < 0) return jspsr::fail(JSPSR_EINVAL, "scene_nearest_seed: negative limit %d (0 = none)", limit);
  int max_h = 0, max_w = 0;
  long long max_items = 0;
  for (int s = 0; s < n_scenes; ++s) {
    const long long off = scenes_host[3 * s], h = scenes_host[3 * s + 1], w = scenes_host[3 * s + 2];
    if (h > kMaxSide || w > kMaxSide)
      return jspsr::fail(JSPSR_EINVAL, "scene_nearest_seed: scene %d is %lld x %lld, sides are at most 32767", s, h, w);
    if (off < 0 || h <= 0 || w <= 0 || off > pixels || h * w > pixels - off)
      return jspsr::fail(JSPSR_EINVAL, "scene_nearest_seed: scene %d (offset %lld, %lld x %lld) leaves the plane of %lld pixels", s,
                         off, h, w, pixels);
    max_h = h > max_h ? (int)h : max_h;
    max_w = w > max_w ? (int)w : max_w;
    const long long items = (h + kBand - 1) / kBand * w;
    max_items = items > max_items ? items : max_items;
  }
  if (!jspsr::aligned4(src) || !jspsr::aligned4(d2) || (reinterpret_cast<uintptr_t>(workspace) & 1u) || !aligned8(scenes))
    return jspsr::fail(JSPSR_EALIGN, "scene_nearest_seed: pointers not aligned to their element size");
  if (limit > 46340) limit = 0;                       // d2 < 2^31 <= limit^2: no bound
  hipStream_t st = static_cast<hipStream_t>(stream);
  short* g = static_cast<short*>(workspace);
  const dim3 grid1(grid_x(max_items), n_scenes < 65535 ? n_scenes : 65535);
  hipLaunchKernelGGL(band_summary_kernel, grid1, dim3(256), 0, st, seed, scenes, n_scenes, pixels, src, d2);
  hipLaunchKernelGGL(column_distance_kernel, grid1, dim3(256), 0, st, seed, scenes, n_scenes, pixels, limit, src, d2, g);
  const size_t lds = ((size_t)max_w * sizeof(short) + 3) / 4 * 4;     // <= 65536
  hipLaunchKernelGGL(row_search_kernel, dim3(max_h, n_scenes < 65535 ? n_scenes : 65535), dim3(256), lds, st, g, scenes,
                     n_scenes, pixels, limit, src, d2);
  return jspsr::check_launch("scene_nearest_seed");
}

extern "C" int jspsr_scene_fill_voids(float* dem, const unsigned char* void_plane, const int* src, long long pixels,
                                      const long long* scenes, int n_scenes, const float* base, jspsr_stream_t stream) {
  if (!dem || !void_plane || !scenes || !base || pixels <= 0 || n_scenes <= 0)
    return jspsr::fail(JSPSR_EINVAL, "scene_fill_voids: bad arguments");
  if (!jspsr::aligned4(dem) || !jspsr::aligned4(src) || !jspsr::aligned4(base) || !aligned8(scenes))
    return jspsr::fail(JSPSR_EALIGN, "scene_fill_voids: pointers not aligned to their element size");
  const int gy = n_scenes < 65535 ? n_scenes : 65535;
  hipLaunchKernelGGL(fill_voids_kernel, dim3(grid_x((pixels + gy - 1) / gy), gy), dim3(256), 0, static_cast<hipStream_t>(stream),
                     dem, void_plane, src, scenes, base, n_scenes, pixels);
  return jspsr::check_launch("scene_fill_voids");
}

extern "C" int jspsr_scene_mask_out(float* out, long long out_len, const unsigned char* void_out, long long pixels,
                                    const long long* rows, int n_rows, float nodata, jspsr_stream_t stream) {
  if (!out || !void_out || !rows || out_len <= 0 || pixels <= 0 || n_rows <= 0)
    return jspsr::fail(JSPSR_EINVAL, "scene_mask_out: bad arguments");
  if (!jspsr::aligned4(out) || !aligned8(rows))
    return jspsr::fail(JSPSR_EALIGN, "scene_mask_out: pointers not aligned to their element size");
  const int gy = n_rows < 65535 ? n_rows : 65535;
  hipLaunchKernelGGL(mask_out_kernel, dim3(grid_x((out_len + gy - 1) / gy), gy), dim3(256), 0, static_cast<hipStream_t>(stream),
                     out, out_len, void_out, pixels, rows, n_rows, nodata);
  return jspsr::check_launch("scene_mask_out");
}
