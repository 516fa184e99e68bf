// K10 -- evaluation scores of a whole BATCH of tiles: what the reference's PerformanceMeter
// computes one tile at a time (valid_batch_size 1) with a meter object per score and a host round trip per value
// (evaluation/evaluate_utils.py:26-47, evaluation/metrics.py), for B tiles per call and with no host synchronisation:
//   * MeterBase._prepare   metrics.py:147-199   border crop by int(h * border), clamp of the prediction to [0, 1]
//   * ToDEM.descale_data   data/data_utils.py:441-457   (the expressions of csrc/metrics.hip, so dh has the same bits)
//   * MeterPSNR "piq"      metrics.py:229-235   -10 log10(mse + 1e-8)
//   * MeterPSNR "local"    metrics.py:97-113    20 log10(1 / sqrt(mse)), 100 at mse == 0
//   * MeterRMSE / MeterMedian / MeterNMAD / MeterLE95   metrics.py:372-384, :453, :508-510, :565-568
//   * MeterSlope "local"   metrics.py:116-139, :670-673   RMS difference of the Sobel magnitudes (valid 3x3, unnormalised)
//   * MeterSlope "kornia"  metrics.py:666-669   RMS of spatial_gradient(P) - spatial_gradient(G): replicate pad, Sobel / 8,
//                          as csrc/train_step.hip restates it; linear, so taken on dh.  Formula-pinned only.
// Two paths, chosen on the host from the cropped size n = h * w:
//   LDS-resident (8 n + 1.6 KiB <= 160 KiB, i.e. up to 142 x 142; covers 128 x 128 at border 0): ONE launch, one
//     1024-thread workgroup per tile.  Both de-scaled rasters are written to LDS once; the sums, the two Sobel terms and
//     the three radix selects (4 passes of a 256-bin integer histogram in LDS each) read them from there.
//   streaming (larger tiles): the multi-pass scheme of csrc/metrics.hip on a (blocks, B) grid with per-tile select state
//     and histogram, plus a slope pass: 27 launches whatever B is.
// Every sum is folded in double in an order that depends on (h, w) only: the same tile gives the same bits in every row
// of every batch size, on every run.
//
// jspsr_scores_batch_valid_forward (K20): the same over the pixels a validity plane (uint8 in the rasters' layout, nonzero =
// valid, cropped with them) keeps.  Every kernel is a template on MASKED; the unmasked instances are K10 as it was.
//   * the flag: after the clamp and the de-scaling the prediction P of a counted pixel is finite (fmaxf / fminf squash a NaN
//     and value_min / value_max are finite), so the first pass writes a NaN into P at a masked pixel and everything after it
//     -- the Sobel pass and the twelve select passes, in LDS and in the streaming workspace alike -- reads the mask from
//     there: no LDS, no workspace and no traffic beyond the plane's one byte per pixel in the first pass.  pred and gt at a
//     masked pixel are loaded but reach a sum or a histogram only behind a select; nothing is multiplied by the mask.
//   * the sums fold in the unmasked order and a masked element adds nothing in place, the path is chosen from (h, w) as in
//     the unmasked call: an all-ones plane gives the unmasked call's bits.
//   * counts {N, N_sl, N_sk} per tile are integers formed on the device (valid pixels; interior positions whose nine taps
//     are valid; positions whose nine replicate-clamped taps are valid); the ranks are K10's formulas of N, formed on the
//     device.  A count of 0 makes its columns NaN and is never turned into a rank: the LDS kernel leaves before the selects
//     (N is uniform over the workgroup), the streaming scan skips its search.
//   * every lane still reaches hist_add; a masked element passes match = false.
//   * launches: 1 (LDS path) or 27 (streaming path) whatever B and the mask are, labels scores_batch_valid (lds | stream).
#include "common.h"
#include "summary_select.h"

#include <cmath>

namespace {

using namespace jspsr;

constexpr int ST = 1024;                      // LDS path: threads per workgroup (16 waves, 4 per SIMD)
constexpr int SW = ST / 64;
constexpr int MT = 256;                       // streaming path
constexpr int NSUM = 4;                       // {sum (p-g)^2, sum dh^2, sum (|grad P| - |grad G|)^2, sum |grad dh / 8|^2}
constexpr int NSCORE = 8;
constexpr int NCNT = 4;                       // K20: {N, N_sl, N_sk, -} per block of the streaming path
constexpr size_t LDS_TOTAL = 163840;          // what one workgroup may declare on gfx950
constexpr size_t LDS_STATIC = 1664;           // hist 1024 + red 4*16*8 = 512 + select state 16, rounded up
constexpr long long LDS_MAX_N = (long long)((LDS_TOTAL - LDS_STATIC) / 8);

__device__ __forceinline__ float descale(float v, float vmin, float vmax, float lg, int elev_log) {
  return elev_log ? expf(v * lg) + vmin : v * (vmax - vmin) + vmin;
}
__device__ __forceinline__ unsigned wave_count(unsigned v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
  return v;
}
// K20's in-band mask: P of a masked pixel is this NaN; P of a counted pixel is finite
__device__ __forceinline__ float masked_flag() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ bool is_masked(float p) { return (__float_as_uint(p) & 0x7fffffffu) > 0x7f800000u; }

// The two Sobel terms of output pixel (y, x) of an h x w pair of de-scaled rasters (row stride w).
//   local:  valid positions only (1 <= y < h-1, 1 <= x < w-1), (|grad P| - |grad G|)^2 with the unnormalised kernels
//   kornia: every position, neighbours clamped to the raster (replicate pad), |grad (P - G) / 8|^2
// MASKED: a position adds its term (and 1 to its count) only where all nine clamped taps are valid, i.e. none of the nine
// P is the flag; at an interior position the clamped taps are the taps, so one test serves both terms.
template <bool MASKED>
__device__ __forceinline__ void sobel_terms(const float* __restrict__ P, const float* __restrict__ G, int h, int w, int y, int x,
                                            double& s_local, double& s_kornia, unsigned& n_local, unsigned& n_kornia) {
  const int ym = y > 0 ? y - 1 : 0, yp = y < h - 1 ? y + 1 : h - 1;
  const int xm = x > 0 ? x - 1 : 0, xp = x < w - 1 ? x + 1 : w - 1;
  const int r0 = ym * w, r1 = y * w, r2 = yp * w;
  const float pa = P[r0 + xm], pb = P[r0 + x], pc = P[r0 + xp], pe = P[r1 + xm], pf = P[r1 + xp], pg = P[r2 + xm], ph = P[r2 + x], pk = P[r2 + xp];
  const float ga = G[r0 + xm], gb = G[r0 + x], gc = G[r0 + xp], ge = G[r1 + xm], gf = G[r1 + xp], gg = G[r2 + xm], gh = G[r2 + x], gk = G[r2 + xp];
  bool all9 = true;
  if constexpr (MASKED)
    all9 = !(is_masked(pa) || is_masked(pb) || is_masked(pc) || is_masked(pe) || is_masked(P[r1 + x]) || is_masked(pf) ||
             is_masked(pg) || is_masked(ph) || is_masked(pk));
  if (all9) {   // spatial_gradient of dh: gx = right - left, gy = below - above, weights 1 2 1, / 8
    const float a = pa - ga, b = pb - gb, c = pc - gc, e = pe - ge, f = pf - gf, g = pg - gg, hh = ph - gh, k = pk - gk;
    const double gx = (double)(((c - a) + 2.f * (f - e) + (k - g)) * 0.125f);
    const double gy = (double)(((g - a) + 2.f * (hh - b) + (k - c)) * 0.125f);
    s_kornia += gx * gx + gy * gy;
    if constexpr (MASKED) ++n_kornia;
  }
  if (all9 && y > 0 && y < h - 1 && x > 0 && x < w - 1) {
    // Gx = [[2,0,-2],[4,0,-4],[2,0,-2]], Gy = [[2,4,2],[0,0,0],[-2,-4,-2]] (cross-correlation): signs drop out of the magnitude
    const float pgx = 2.f * (pa - pc) + 4.f * (pe - pf) + 2.f * (pg - pk), pgy = 2.f * (pa - pg) + 4.f * (pb - ph) + 2.f * (pc - pk);
    const float ggx = 2.f * (ga - gc) + 4.f * (ge - gf) + 2.f * (gg - gk), ggy = 2.f * (ga - gg) + 4.f * (gb - gh) + 2.f * (gc - gk);
    const double d = (double)sqrtf(pgx * pgx + pgy * pgy) - (double)sqrtf(ggx * ggx + ggy * ggy);
    s_local += d * d;
    if constexpr (MASKED) ++n_local;
  }
}

// scores 0, 1, 2, 6, 7 of one tile from its four sums
__device__ __forceinline__ void write_sum_scores(const double* s, int h, int w, float* __restrict__ out) {
  const double n = (double)h * (double)w;
  const double mse = s[0] / n;
  out[0] = (float)(-10.0 * log10(mse + 1e-8));
  out[1] = mse == 0.0 ? 100.f : (float)(20.0 * log10(1.0 / sqrt(mse)));
  out[2] = (float)sqrt(s[1] / n);
  out[6] = (float)sqrt(s[2] / ((double)(h - 2) * (double)(w - 2)));
  out[7] = (float)sqrt(s[3] / (2.0 * n));
}
// K20: the same from the tile's counts c = {N, N_sl, N_sk} (the unmasked divisors when everything is valid); a column
// whose count is 0 is NaN by a select, not by a division
__device__ __forceinline__ void write_sum_scores_valid(const double* s, const unsigned* c, float* __restrict__ out,
                                                       int* __restrict__ counts) {
  const float nan = masked_flag();
  const double n = (double)c[0], n_sl = (double)c[1], n_sk = (double)c[2];
  const double mse = s[0] / (c[0] ? n : 1.0);
  out[0] = c[0] ? (float)(-10.0 * log10(mse + 1e-8)) : nan;
  out[1] = c[0] ? (mse == 0.0 ? 100.f : (float)(20.0 * log10(1.0 / sqrt(mse)))) : nan;
  out[2] = c[0] ? (float)sqrt(s[1] / n) : nan;
  out[6] = c[1] ? (float)sqrt(s[2] / n_sl) : nan;
  out[7] = c[2] ? (float)sqrt(s[3] / (2.0 * n_sk)) : nan;
  counts[0] = (int)c[0];
  counts[1] = (int)c[1];
  counts[2] = (int)c[2];
}
__device__ __forceinline__ unsigned rank_median(long long n) { return (unsigned)((n - 1) / 2); }                       // lower median, 0-based
__device__ __forceinline__ unsigned rank_le95(long long n) { return (unsigned)llrint(0.95 * (double)(n - 1)); }       // 1 + round(0.95 (n-1)), 0-based

// ---- LDS-resident path ---------------------------------------------------------------------------------------------
template <bool MASKED>
__global__ __launch_bounds__(ST) void scores_lds_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       const unsigned char* __restrict__ valid, int H, int W,
                                                       int bh, int bw, float vmin, float vmax, int elev_log,
                                                       float* __restrict__ scores, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float rast[];   // P[n] | G[n], de-scaled
  __shared__ unsigned hist[256];
  __shared__ double red[NSUM][SW];
  __shared__ unsigned sel_prefix, sel_k;
  __shared__ float sel_center;
  __shared__ unsigned sel_n;                                     // MASKED: the tile's N
  const int h = H - 2 * bh, w = W - 2 * bw, n = h * w;
  float* P = rast;
  float* G = rast + n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t tile = (size_t)blockIdx.x * H * W;
  float* out = scores + (size_t)blockIdx.x * NSCORE;
  const float lg = logf(vmax - vmin);
  double s[2] = {0.0, 0.0};
  unsigned c[2] = {0u, 0u};                                      // MASKED: this lane's counts (hist is free until the selects)
  for (int y = wave; y < h; y += SW) {                           // a wave per row: coalesced reads, no division
    const size_t src = tile + (size_t)(y + bh) * W + bw;
#pragma unroll 1
    for (int x = lane; x < w; x += 64) {
      bool ok = true;
      if constexpr (MASKED) ok = valid[src + x] != 0;
      const float p = fminf(fmaxf(pred[src + x], 0.f), 1.f), g = gt[src + x];
      const float dp = descale(p, vmin, vmax, lg, elev_log), dg = descale(g, vmin, vmax, lg, elev_log);
      P[y * w + x] = ok ? dp : masked_flag();
      G[y * w + x] = dg;
      const double e = (double)p - (double)g, d = (double)(dp - dg);
      if (ok) {
        s[0] += e * e;
        s[1] += d * d;
        if constexpr (MASKED) ++c[0];
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double v = wave_sum(s[q]);
    if (lane == 0) red[q][wave] = v;
  }
  if constexpr (MASKED) {
    const unsigned v = wave_count(c[0]);
    if (lane == 0) hist[wave] = v;
  }
  __syncthreads();
  s[0] = s[1] = 0.0;
  c[0] = c[1] = 0u;
  for (int y = wave; y < h; y += SW) {
#pragma unroll 1
    for (int x = lane; x < w; x += 64) sobel_terms<MASKED>(P, G, h, w, y, x, s[0], s[1], c[0], c[1]);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double v = wave_sum(s[q]);
    if (lane == 0) red[2 + q][wave] = v;
  }
  if constexpr (MASKED) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const unsigned v = wave_count(c[q]);
      if (lane == 0) hist[(1 + q) * SW + wave] = v;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double t[NSUM];
    for (int q = 0; q < NSUM; ++q) {
      t[q] = 0.0;
      for (int k = 0; k < SW; ++k) t[q] += red[q][k];
    }
    if constexpr (MASKED) {
      unsigned ct[3];
      for (int q = 0; q < 3; ++q) {
        ct[q] = 0u;
        for (int k = 0; k < SW; ++k) ct[q] += hist[q * SW + k];
      }
      write_sum_scores_valid(t, ct, out, counts + (size_t)blockIdx.x * 3);
      sel_n = ct[0];
    } else {
      write_sum_scores(t, h, w, out);
    }
  }
  unsigned n_valid = (unsigned)n;
  if constexpr (MASKED) {
    __syncthreads();                                             // thread 0 has read the counts out of hist; N for everyone
    n_valid = sel_n;
    if (n_valid == 0u) {                                         // uniform over the workgroup: no rank is formed from N = 0
      if (tid == 0) out[3] = out[4] = out[5] = masked_flag();
      return;
    }
  }
  // three exact order statistics: median of dh, median of |dh - median|, k-th of |dh|
  for (int q = 0; q < 3; ++q) {
    if (tid == 0) {
      sel_prefix = 0u;
      sel_k = q == 2 ? rank_le95(n_valid) : rank_median(n_valid);
      if (q == 0) sel_center = 0.f;
    }
    for (int pass = 3; pass >= 0; --pass) {
      if (tid < 256) hist[tid] = 0u;
      __syncthreads();
      const unsigned prefix = sel_prefix;
      const float center = sel_center;
      const int shift = pass * 8;
      const unsigned himask = pass == 3 ? 0u : (0xffffffffu << (shift + 8));
      for (int base = 0; base < n; base += ST) {                 // wave-uniform trip count (hist_add uses ballots)
        const int i = base + tid;
        bool match = i < n;
        unsigned bin = 0u;
        if (match) {
          const float pi = P[i];
          const unsigned key = order_key(sel_transform(pi - G[i], q, center));
          match = (key & himask) == (prefix & himask);
          if constexpr (MASKED) match = match && !is_masked(pi);  // a masked element reaches hist_add with match = false
          bin = (key >> shift) & 0xffu;
        }
        hist_add(hist, match, bin);
      }
      __syncthreads();
      if (wave == 0) {                                           // lane l owns bins 4l .. 4l+3
        const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        const unsigned own = c0 + c1 + c2 + c3;
        unsigned incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned up = (unsigned)__shfl_up((int)incl, d, 64);
          if (lane >= d) incl += up;
        }
        const unsigned k = sel_k, excl = incl - own;
        if (k >= excl && k < incl) {                             // exactly one lane: the counts sum to more than k (N >= 1)
          unsigned run = excl;
          int b = 0;
          if (k >= run + c0) { run += c0; b = 1;
            if (k >= run + c1) { run += c1; b = 2;
              if (k >= run + c2) { run += c2; b = 3; } } }
          sel_k = k - run;
          sel_prefix = prefix | ((unsigned)(4 * lane + b) << shift);
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const float v = key_value(sel_prefix);
      out[3 + q] = q == 1 ? v * 1.4826f : v;
      if (q == 0) sel_center = v;
    }
    __syncthreads();
  }
}

// ---- streaming path ------------------------------------------------------------------------------------------------
struct SelState {          // one per (tile, statistic), in device memory
  unsigned prefix;         // key bits fixed so far (high bits)
  unsigned k;              // rank still to find inside the current prefix class (0-based)
  float center;            // mode 1: |x - center|
  unsigned n;              // MASKED: the tile's N (0: no rank, the scan writes NaN); unmasked: unused
};

__device__ __forceinline__ void block_partials(double* s, int count, double* __restrict__ dst) {
  __shared__ double red[NSUM][MT / 64];
  for (int q = 0; q < count; ++q) {
    const double v = wave_sum(s[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < count) {
    double t = 0.0;
    for (int k = 0; k < MT / 64; ++k) t += red[threadIdx.x][k];
    dst[threadIdx.x] = t;
  }
}
// K20: the workgroup's integer counts -> dst[first .. first + count)
__device__ __forceinline__ void block_counts(const unsigned* c, int count, unsigned* __restrict__ dst) {
  __shared__ unsigned cred[2][MT / 64];
  for (int q = 0; q < count; ++q) {
    const unsigned v = wave_count(c[q]);
    if ((threadIdx.x & 63) == 0) cred[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < count) {
    unsigned t = 0u;
    for (int k = 0; k < MT / 64; ++k) t += cred[threadIdx.x][k];
    dst[threadIdx.x] = t;
  }
}

// de-scaled rasters P, G [B][n] and the per-block sums {sum (p-g)^2, sum dh^2} -> partial[b][block][0..1]
// MASKED: P = the flag at a masked pixel; the block's N -> cpart[b][block][0]
template <bool MASKED>
__global__ __launch_bounds__(MT) void scores_prepare_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const unsigned char* __restrict__ valid, int H, int W,
                                                           int bh, int bw, float vmin, float vmax, int elev_log,
                                                           float* __restrict__ P, float* __restrict__ G, double* __restrict__ partial,
                                                           unsigned* __restrict__ cpart) {
  const int h = H - 2 * bh, w = W - 2 * bw;
  const long long n = (long long)h * w;
  const size_t tile = (size_t)blockIdx.y * H * W, dst = (size_t)blockIdx.y * n;
  const float lg = logf(vmax - vmin);
  double s[2] = {0.0, 0.0};
  unsigned c[1] = {0u};
  for (long long i = blockIdx.x * (long long)MT + threadIdx.x; i < n; i += (long long)gridDim.x * MT) {
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    const size_t j = tile + (size_t)(y + bh) * W + (x + bw);
    bool ok = true;
    if constexpr (MASKED) ok = valid[j] != 0;
    const float p = fminf(fmaxf(pred[j], 0.f), 1.f), g = gt[j];
    const float dp = descale(p, vmin, vmax, lg, elev_log), dg = descale(g, vmin, vmax, lg, elev_log);
    P[dst + i] = ok ? dp : masked_flag();
    G[dst + i] = dg;
    const double e = (double)p - (double)g, d = (double)(dp - dg);
    if (ok) {
      s[0] += e * e;
      s[1] += d * d;
      if constexpr (MASKED) ++c[0];
    }
  }
  block_partials(s, 2, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NSUM);
  if constexpr (MASKED) block_counts(c, 1, cpart + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NCNT);
}

// the two Sobel sums -> partial[b][block][2..3]; MASKED: their counts -> cpart[b][block][1..2]
template <bool MASKED>
__global__ __launch_bounds__(MT) void scores_slope_kernel(const float* __restrict__ P, const float* __restrict__ G, int h, int w,
                                                         double* __restrict__ partial, unsigned* __restrict__ cpart) {
  const long long n = (long long)h * w;
  const float* p = P + (size_t)blockIdx.y * n;
  const float* g = G + (size_t)blockIdx.y * n;
  double s[2] = {0.0, 0.0};
  unsigned c[2] = {0u, 0u};
  for (long long i = blockIdx.x * (long long)MT + threadIdx.x; i < n; i += (long long)gridDim.x * MT) {
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    sobel_terms<MASKED>(p, g, h, w, y, x, s[0], s[1], c[0], c[1]);
  }
  block_partials(s, 2, partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NSUM + 2);
  if constexpr (MASKED) block_counts(c, 2, cpart + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NCNT + 1);
}

// one workgroup per tile: scores 0, 1, 2, 6, 7 from the partial rows (fixed order); initialises the tile's select states
// MASKED: the tile's counts from cpart (integers: any order), its ranks from N
template <bool MASKED>
__global__ __launch_bounds__(MT) void scores_reduce_kernel(const double* __restrict__ partial, const unsigned* __restrict__ cpart, int rows,
                                                          int h, int w, float* __restrict__ scores, int* __restrict__ counts,
                                                          SelState* __restrict__ st, unsigned* __restrict__ hist) {
  __shared__ double red[NSUM][MT / 64];
  __shared__ unsigned ctot[3];
  if constexpr (MASKED) {
    if (threadIdx.x < 3) ctot[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned* csrc = cpart + (size_t)blockIdx.x * rows * NCNT;
    unsigned c[3] = {0u, 0u, 0u};
    for (int i = threadIdx.x; i < rows; i += MT)
      for (int q = 0; q < 3; ++q) c[q] += csrc[(size_t)i * NCNT + q];
    for (int q = 0; q < 3; ++q) {
      const unsigned v = wave_count(c[q]);
      if ((threadIdx.x & 63) == 0) atomicAdd(&ctot[q], v);
    }
  }
  const double* src = partial + (size_t)blockIdx.x * rows * NSUM;
  double s[NSUM] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < rows; i += MT)
    for (int q = 0; q < NSUM; ++q) s[q] += src[(size_t)i * NSUM + q];
  for (int q = 0; q < NSUM; ++q) {
    const double v = wave_sum(s[q]);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[NSUM];
    for (int q = 0; q < NSUM; ++q) {
      t[q] = 0.0;
      for (int k = 0; k < MT / 64; ++k) t[q] += red[q][k];
    }
    SelState* s3 = st + (size_t)blockIdx.x * 3;
    if constexpr (MASKED) {
      const unsigned ct[3] = {ctot[0], ctot[1], ctot[2]};
      write_sum_scores_valid(t, ct, scores + (size_t)blockIdx.x * NSCORE, counts + (size_t)blockIdx.x * 3);
      const unsigned nv = ct[0];                       // N = 0: no rank is formed, the scan writes NaN
      s3[0] = SelState{0u, nv ? rank_median(nv) : 0u, 0.f, nv};
      s3[1] = SelState{0u, nv ? rank_median(nv) : 0u, 0.f, nv};
      s3[2] = SelState{0u, nv ? rank_le95(nv) : 0u, 0.f, nv};
    } else {
      write_sum_scores(t, h, w, scores + (size_t)blockIdx.x * NSCORE);
      const long long n = (long long)h * w;
      s3[0] = SelState{0u, rank_median(n), 0.f, 0u};
      s3[1] = SelState{0u, rank_median(n), 0.f, 0u};    // center filled in after statistic 0
      s3[2] = SelState{0u, rank_le95(n), 0.f, 0u};
    }
  }
  for (int i = threadIdx.x; i < 256; i += MT) hist[(size_t)blockIdx.x * 256 + i] = 0u;
}

// histogram of byte `pass` (3 = most significant) of the keys of tile blockIdx.y whose higher bytes equal its prefix
template <bool MASKED>
__global__ __launch_bounds__(MT) void scores_hist_kernel(const float* __restrict__ P, const float* __restrict__ G, long long n, int q,
                                                        int pass, const SelState* __restrict__ st, unsigned* __restrict__ hist) {
  __shared__ unsigned lh[256];
  lh[threadIdx.x] = 0u;
  __syncthreads();
  const SelState* my = st + (size_t)blockIdx.y * 3 + q;
  const unsigned prefix = my->prefix;
  const float center = my->center;
  const float* p = P + (size_t)blockIdx.y * n;
  const float* g = G + (size_t)blockIdx.y * n;
  const int shift = pass * 8;
  const unsigned himask = pass == 3 ? 0u : (0xffffffffu << (shift + 8));
  for (long long i = blockIdx.x * (long long)MT + threadIdx.x; i < n; i += (long long)gridDim.x * MT) {
    const float pi = p[i];
    const unsigned key = order_key(sel_transform(pi - g[i], q, center));
    bool match = (key & himask) == (prefix & himask);
    if constexpr (MASKED) match = match && !is_masked(pi);
    if (match) atomicAdd(&lh[(key >> shift) & 0xffu], 1u);
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&hist[(size_t)blockIdx.y * 256 + threadIdx.x], lh[threadIdx.x]);
}

// one workgroup per tile: find the bin holding rank k, fix its byte, reduce k, clear the histogram; after the last pass
// write the value to the tile's score and, for the median, hand it to the NMAD select as its center.  MASKED: a tile with
// N = 0 searches nothing and gets NaN
template <bool MASKED>
__global__ __launch_bounds__(256) void scores_scan_kernel(unsigned* __restrict__ hist, int q, int pass, SelState* __restrict__ st,
                                                         float* __restrict__ scores) {
  __shared__ unsigned cum[256];
  unsigned* hb = hist + (size_t)blockIdx.x * 256;
  cum[threadIdx.x] = hb[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    SelState* s3 = st + (size_t)blockIdx.x * 3;
    if (MASKED && s3[q].n == 0u) {
      if (pass == 0) scores[(size_t)blockIdx.x * NSCORE + 3 + q] = masked_flag();
    } else {
      unsigned run = 0, k = s3[q].k;
      int bin = 255;
      for (int b = 0; b < 256; ++b) {
        if (k < run + cum[b]) { bin = b; break; }
        run += cum[b];
      }
      s3[q].k = k - run;
      s3[q].prefix |= (unsigned)bin << (pass * 8);
      if (pass == 0) {
        const float v = key_value(s3[q].prefix);
        scores[(size_t)blockIdx.x * NSCORE + 3 + q] = q == 1 ? v * 1.4826f : v;
        if (q == 0) s3[1].center = v;
      }
    }
  }
  hb[threadIdx.x] = 0u;
}

int stream_blocks(long long n) {
  long long b = (n + MT * 8 - 1) / (MT * 8);
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

size_t workspace_bytes(bool masked, int B, int H, int W) {
  if (B <= 0 || H < 3 || W < 3) return 0;                // what scores_run refuses whatever the border is: 0, as documented
  const long long n = (long long)H * W;
  if (n > 0x7fffffffLL / 2) return 0;
  if (n <= LDS_MAX_N) return 16;                         // LDS path for every border: nothing is staged in memory
  // every region below is a multiple of 16 bytes but the two planes; the + 64 is spare (it covers no rounding)
  return 2 * up16((size_t)B * n * sizeof(float)) + up16((size_t)B * stream_blocks(n) * NSUM * sizeof(double)) +
         (size_t)B * 256 * sizeof(unsigned) + up16((size_t)B * 3 * sizeof(SelState)) + 64 +
         (masked ? up16((size_t)B * stream_blocks(n) * NCNT * sizeof(unsigned)) : 0);
}

template <bool MASKED>
int scores_run(const char* name, const float* pred, const float* gt, const unsigned char* valid, int B, int H, int W, float border,
               float value_min, float value_max, int elev_log, float* scores, int* counts, void* workspace, jspsr_stream_t stream) {
  if (!pred || !gt || !scores || !workspace || B <= 0 || H <= 0 || W <= 0) return fail(JSPSR_EINVAL, "%s: bad arguments", name);
  if (MASKED && (!valid || !counts)) return fail(JSPSR_EINVAL, "%s: null validity plane or counts", name);
  if (!(border >= 0.f) || border >= 0.5f) return fail(JSPSR_EINVAL, "%s: border must be in [0, 0.5)", name);
  if (!(value_max - value_min > 1.f)) return fail(JSPSR_EINVAL, "%s: value_max - value_min must exceed 1", name);
  if ((long long)H * W > 0x7fffffffLL / 2) return fail(JSPSR_EINVAL, "%s: tile of %d x %d is too large", name, H, W);
  if (!aligned4(pred) || !aligned4(gt) || !aligned4(scores)) return fail(JSPSR_EALIGN, "%s: tensors not 4-byte aligned", name);
  if (MASKED && !aligned4(counts)) return fail(JSPSR_EALIGN, "%s: counts not 4-byte aligned", name);
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "%s: workspace not 16-byte aligned", name);
  const int bh = (int)((float)H * border), bw = (int)((float)W * border);     // int(h * border), metrics.py:172-183
  const int h = H - 2 * bh, w = W - 2 * bw;
  if (h <= 0 || w <= 0) return fail(JSPSR_EINVAL, "%s: nothing left after the border crop", name);
  if (h < 3 || w < 3) return fail(JSPSR_EINVAL, "%s: %d x %d left after the crop, the slope needs 3 x 3", name, h, w);
  const long long n = (long long)h * w;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n <= LDS_MAX_N) {                                   // the path depends on (h, w) only, never on the mask
    const size_t lds = (size_t)n * 2 * sizeof(float);
    static_assert(LDS_MAX_N * 8 + LDS_STATIC <= LDS_TOTAL, "LDS budget");
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scores_lds_kernel<MASKED>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(LDS_TOTAL - LDS_STATIC));
    hipLaunchKernelGGL(scores_lds_kernel<MASKED>, dim3(B), dim3(ST), lds, s, pred, gt, valid, H, W, bh, bw, value_min, value_max,
                       elev_log, scores, counts);
    return check_launch(MASKED ? "scores_batch_valid (lds)" : "scores_batch (lds)");
  }
  if (B > 65535) return fail(JSPSR_EINVAL, "%s: B = %d exceeds the streaming path's grid (65535)", name, B);
  const char* const label = MASKED ? "scores_batch_valid (stream)" : "scores_batch (stream)";
  const int blocks = stream_blocks(n);
  char* ws = static_cast<char*>(workspace);
  const size_t plane = up16((size_t)B * H * W * sizeof(float));    // laid out for the uncropped size, as the size query is
  float* P = reinterpret_cast<float*>(ws);
  float* G = reinterpret_cast<float*>(ws + plane);
  size_t off = 2 * plane;
  double* partial = reinterpret_cast<double*>(ws + off);
  off += up16((size_t)B * stream_blocks((long long)H * W) * NSUM * sizeof(double));
  unsigned* hist = reinterpret_cast<unsigned*>(ws + off);
  off += (size_t)B * 256 * sizeof(unsigned);
  SelState* st = reinterpret_cast<SelState*>(ws + off);
  off += up16((size_t)B * 3 * sizeof(SelState));
  unsigned* cpart = MASKED ? reinterpret_cast<unsigned*>(ws + off) : nullptr;   // B * blocks * NCNT, blocks <= stream_blocks(H W)
  hipLaunchKernelGGL(scores_prepare_kernel<MASKED>, dim3(blocks, B), dim3(MT), 0, s, pred, gt, valid, H, W, bh, bw, value_min, value_max,
                     elev_log, P, G, partial, cpart);
  if (int e = check_launch(label)) return e;
  hipLaunchKernelGGL(scores_slope_kernel<MASKED>, dim3(blocks, B), dim3(MT), 0, s, P, G, h, w, partial, cpart);
  if (int e = check_launch(label)) return e;
  hipLaunchKernelGGL(scores_reduce_kernel<MASKED>, dim3(B), dim3(MT), 0, s, partial, cpart, blocks, h, w, scores, counts, st, hist);
  if (int e = check_launch(label)) return e;
  for (int q = 0; q < 3; ++q) {
    for (int pass = 3; pass >= 0; --pass) {
      hipLaunchKernelGGL(scores_hist_kernel<MASKED>, dim3(blocks, B), dim3(MT), 0, s, P, G, n, q, pass, st, hist);
      if (int e = check_launch(label)) return e;
      hipLaunchKernelGGL(scores_scan_kernel<MASKED>, dim3(B), dim3(256), 0, s, hist, q, pass, st, scores);
      if (int e = check_launch(label)) return e;
    }
  }
  return JSPSR_OK;
}

}  // namespace

extern "C" size_t jspsr_scores_batch_workspace_bytes(int B, int H, int W) { return workspace_bytes(false, B, H, W); }

extern "C" int jspsr_scores_batch_forward(const float* pred, const float* gt, int B, int H, int W, float border, float value_min,
                                          float value_max, int elev_log, float* scores, void* workspace, jspsr_stream_t stream) {
  return scores_run<false>("scores_batch_forward", pred, gt, nullptr, B, H, W, border, value_min, value_max, elev_log, scores, nullptr,
                           workspace, stream);
}

extern "C" size_t jspsr_scores_batch_valid_workspace_bytes(int B, int H, int W) { return workspace_bytes(true, B, H, W); }

extern "C" int jspsr_scores_batch_valid_forward(const float* pred, const float* gt, const unsigned char* valid, int B, int H, int W,
                                                float border, float value_min, float value_max, int elev_log, float* scores,
                                                int* counts, void* workspace, jspsr_stream_t stream) {
  return scores_run<true>("scores_batch_valid_forward", pred, gt, valid, B, H, W, border, value_min, value_max, elev_log, scores, counts,
                          workspace, stream);
}
