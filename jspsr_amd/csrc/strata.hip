// K22 -- whole-set scores by terrain class: K12's eleven-column row for every candidate and
// every class of a uint8 label plane in the ground truth's layout, from one pool, and the slope-class plane such a table is
// usually cut by.
// (a) jspsr_strata_forward: K18's streaming selection with one row state per (candidate, class) instead of per (candidate,
//     segment).  The pool is cut into fixed RUNs of 8192 elements, a workgroup owns one RUN of one candidate:
//       prepare   reads the candidate, the ground truth, the labels and the optional validity plane through the window
//                 table; writes e = cand - gt once per candidate and the class byte once (255: belongs to no class); folds
//                 e^2 in double per (RUN, class) -- a column of LDS doubles per thread and class, reduced in K18's order -- and
//                 counts the top digit of the keys of e and |e| into per-class LDS histograms;
//       select    8 bits per pass, every pass serving ALL classes at once: n_classes x {4, 2} x 256 LDS counters (the two
//                 ranks of a statistic are two states whose prefixes may diverge), the class of an element picks the
//                 histogram and the prefixes it is compared with (kept in LDS, read per lane);
//       scan      a workgroup per (candidate, class): rank_scan (summary_select.h), the scan K12 and K18 run, behind an
//                 init block of its own.  The class count n_c is the sum of the class's top-digit histogram of e
//                 (integers, exact), so the ranks, the LE95 weight and the divisor of the sum are formed there by
//                 segment_ranks_of, the inline K18 uses.
//     The window reader (pooled_fetch), the candidates' Buffers and their check are csrc/pooled_read.h's; the labels and
//     the validity plane are this kernel's own arguments, read at the ground truth's index the reader hands over.
//     16 launches whatever n_classes, n_cand, the windows and the data are.  Integer adds only in the histograms, and every
//     fp64 sum is folded in an order the pool's size alone fixes: a row has the same bits for every n_cand, whatever the
//     other classes hold, on every run.  Hot counters take hist_add's ballot-aggregated increments: one class routinely
//     holds most of a scene.  The LDS a workgroup takes grows with n_classes (4 KiB per class in prepare and in the first
//     group's selects, 2 KiB in the second's; 128 KiB at 32 classes, one workgroup per CU): that, not the traffic, is what
//     the cost of many classes is made of.
// (b) jspsr_slope_classes: ONE launch, a thread per pixel of the plane.  The scene of a pixel is found by bisection in the
//     scene table; the nine taps are replicate-clamped inside that scene; Sobel in single roundings (explicit __f*_rn and
//     -ffp-contract=off), p = gx^2 + gy^2 compared with the caller's thresholds: no atan on the device.
#include "common.h"
#include "pooled_read.h"
#include "summary_select.h"

#include <cmath>

namespace {

using namespace jspsr;

constexpr int MT = SCAN_MT;
constexpr int UNROLL = 4;
constexpr int RUN = 8192;                     // pooled elements per workgroup and per fp64 partial sum (jspsr_amd/summary.py: CHUNK)
constexpr int MAXK = 32;                      // classes
constexpr int NONE = 255;                     // the class byte of an element that belongs to no class
constexpr int MAXT = 31;                      // slope thresholds
static_assert(RUN % (MT * UNROLL) == 0, "a run is a whole number of unrolled steps");

// labels, valid: planes in gt's layout and numel (checked by the entry); valid may be null
// LDS of prepare: n_classes x { 2 x 256 counters, 256 doubles }; of select: n_classes x slots x 256 counters
__global__ __launch_bounds__(MT) void strata_prepare_kernel(Buffers B, const unsigned char* __restrict__ labels,
                                                           const unsigned char* __restrict__ valid, const long long* __restrict__ win,
                                                           int n_win, long long total, long long n_runs, int n_classes, int reps,
                                                           float* __restrict__ e_all, unsigned char* __restrict__ cls_all,
                                                           double* __restrict__ partial, unsigned* __restrict__ hist) {
  extern __shared__ double dyn[];
  __shared__ double red[MAXK][MT / 64];
  double* __restrict__ sums = dyn;                                            // [n_classes][MT]
  unsigned* __restrict__ lh = reinterpret_cast<unsigned*>(dyn + (size_t)n_classes * MT);   // [n_classes][2][256]
  const int tid = threadIdx.x, c = blockIdx.y;
  for (int i = tid; i < n_classes * MT; i += MT) sums[i] = 0.0;
  for (int i = tid; i < n_classes * 512; i += MT) lh[i] = 0u;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * RUN;
  const long long hi = lo + RUN < total ? lo + RUN : total;                   // lo < total: the grid is n_runs wide
  float* __restrict__ e = e_all + (size_t)c * total;
  WindowCursor W(B, c);
  for (long long base = lo; base < hi; base += MT * UNROLL) {
    float err[UNROLL];
    int cls[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long long p = base + u * MT + tid;
      cls[u] = NONE;
      err[u] = 0.f;
      if (p >= hi) continue;
      float v;                                                  // a NaN: an element no window covers, or a read outside a buffer:
      int k = 0;                                                // ... of class 0, so that a bad table shows (K12 does the same)
      pooled_fetch(W, win, n_win, p, v, [&](long long jg) {
        k = labels[jg];
        if (k >= n_classes) k = NONE;
        if (valid != nullptr && valid[jg] == 0) k = NONE;
      });
      if (k == NONE) v = 0.f;                                     // whatever cand and gt hold there: it is never looked at again
      cls[u] = k;
      err[u] = v;
      e[p] = v;
      if (c == 0) cls_all[p] = (unsigned char)k;
      if (k != NONE) sums[k * MT + tid] += (double)v * (double)v;  // this thread's own column: no other thread adds to it
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const bool m = cls[u] != NONE;
      const unsigned row = m ? (unsigned)cls[u] * 512u : 0u;
      hist_add(lh, m, row + (order_key(err[u]) >> 24));
      hist_add(lh, m, row + 256u + (order_key(fabsf(err[u])) >> 24));
    }
  }
  __syncthreads();
  // the run's sum per class, in the order K18 folds a chunk: a wave's 64 columns by the butterfly, then the four waves
  for (int k = 0; k < n_classes; ++k) {
    const double v = wave_sum(sums[k * MT + tid]);
    if ((tid & 63) == 0) red[k][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < n_classes) {
    double t = 0.0;
    for (int q = 0; q < MT / 64; ++q) t += red[tid][q];
    partial[((size_t)c * n_runs + blockIdx.x) * n_classes + tid] = t;
  }
  const int rep = (int)(blockIdx.x & (unsigned)(reps - 1));      // reps is a power of two
  for (int i = tid; i < n_classes * 512; i += MT) {
    const unsigned v = lh[i];
    if (!v) continue;
    const int k = i >> 9, q = (i >> 8) & 1, b = i & 255;          // q = 1: |e|, state 2
    atomicAdd(&hist[((((size_t)c * n_classes + k) * reps + rep) * NSTATE + 2 * q) * 256 + b], v);
  }
}

// histograms of byte `pass` of the keys that carry their state's prefix, for every class.  group 0: states 0..3 (e and
// |e|, one read for both); group 1: states 4, 5 (|e - median|).  While the two states of a pair agree on the higher bytes,
// only the lower one is counted (the scan reads it for both).
__global__ __launch_bounds__(MT) void strata_select_kernel(const float* __restrict__ e_all, const unsigned char* __restrict__ cls_all,
                                                          long long total, int n_classes, int reps, int group, int pass,
                                                          const RowState* __restrict__ st, unsigned* __restrict__ hist) {
  extern __shared__ double dyn[];
  __shared__ unsigned pfx[4][MAXK];
  __shared__ float centers[MAXK];
  unsigned* __restrict__ lh = reinterpret_cast<unsigned*>(dyn);  // [n_classes][slots][256]
  const int tid = threadIdx.x, c = blockIdx.y;
  const int slots = group ? 2 : 4, q0 = group ? 4 : 0;
  const int shift = pass * 8;
  const unsigned himask = pass == 3 ? 0u : (0xffffffffu << (shift + 8));
  for (int i = tid; i < n_classes * slots * 256; i += MT) lh[i] = 0u;
  if (tid < n_classes) {
    const RowState* my = st + (size_t)c * n_classes + tid;
    pfx[0][tid] = my->prefix[q0] & himask;
    pfx[1][tid] = my->prefix[q0 + 1] & himask;
    pfx[2][tid] = group ? 0u : my->prefix[2] & himask;
    pfx[3][tid] = group ? 0u : my->prefix[3] & himask;
    centers[tid] = my->center;
  }
  __syncthreads();
  const long long lo = (long long)blockIdx.x * RUN;
  const long long hi = lo + RUN < total ? lo + RUN : total;
  const float* __restrict__ e = e_all + (size_t)c * total;
  for (long long base = lo; base < hi; base += MT * UNROLL) {
    float x[UNROLL];
    int cls[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long long p = base + u * MT + tid;
      const bool in = p < hi;
      x[u] = in ? e[p] : 0.f;
      cls[u] = in ? (int)cls_all[p] : NONE;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const bool m = cls[u] != NONE;
      const int k = m ? cls[u] : 0;
      const unsigned row = (unsigned)(k * slots) * 256u;
      const unsigned pa0 = pfx[0][k], pa1 = pfx[1][k];
      const unsigned ka = order_key(group ? fabsf(__fsub_rn(x[u], centers[k])) : x[u]);
      const unsigned bin_a = (ka >> shift) & 0xffu;
      hist_add(lh, m && (ka & himask) == pa0, row + bin_a);
      hist_add(lh, m && pa0 != pa1 && (ka & himask) == pa1, row + 256u + bin_a);
      if (!group) {                                              // kernel-uniform
        const unsigned pb0 = pfx[2][k], pb1 = pfx[3][k];
        const unsigned kb = order_key(fabsf(x[u]));
        const unsigned bin_b = (kb >> shift) & 0xffu;
        hist_add(lh, m && (kb & himask) == pb0, row + 512u + bin_b);
        hist_add(lh, m && pb0 != pb1 && (kb & himask) == pb1, row + 768u + bin_b);
      }
    }
  }
  __syncthreads();
  const int rep = (int)(blockIdx.x & (unsigned)(reps - 1));
  for (int i = tid; i < n_classes * slots * 256; i += MT) {
    const unsigned v = lh[i];
    if (!v) continue;
    const int k = i / (slots * 256), q = (i >> 8) % slots, b = i & 255;
    atomicAdd(&hist[((((size_t)c * n_classes + k) * reps + rep) * NSTATE + q0 + q) * 256 + b], v);
  }
}

// One workgroup per (candidate, class): rank_scan (summary_select.h) behind this kernel's own init block.  init: the
// first scan of a call -- n_c from the class's top-digit histogram of e, the ranks formed from it, RMSE / PSNR from the
// run sums.
__global__ __launch_bounds__(MT) void strata_scan_kernel(const double* __restrict__ partial, long long n_runs, int n_classes, int reps,
                                                        int group, int pass, int init, double value_max, RowState* __restrict__ st,
                                                        unsigned* __restrict__ hist, float* __restrict__ out,
                                                        long long* __restrict__ counts) {
  __shared__ RowState cur;
  __shared__ double red[MT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row = blockIdx.x;
  const int c = (int)(row / n_classes), cl = (int)(row % n_classes);
  unsigned* hrow = hist + row * reps * NSTATE * 256;           // the row's `reps` replicas, back to back
  float* o = out + row * NOUT;
  long long n_v = 0;
  if (init) {
    if (tid == 0) {
      for (int q = 0; q < NSTATE; ++q) cur.prefix[q] = 0u;
      cur.center = 0.f;
      cur.has_nan = 0u;
      cur.g[0] = cur.g[1] = 0u;
    }
    const double* src = partial + (size_t)c * n_runs * n_classes + cl;
    double a = 0.0;
    for (long long j = tid; j < n_runs; j += MT) a += src[(size_t)j * n_classes];
    a = wave_sum(a);
    if (lane == 0) red[wave] = a;
    // n_c: every counted element of the class is in exactly one bin of its top-digit histogram of e.  Every wave forms it.
    for (int r = 0; r < reps; ++r) {
      const uint4 v = *reinterpret_cast<const uint4*>(hrow + (size_t)r * NSTATE * 256 + 4 * lane);
      n_v += (long long)v.x + v.y + v.z + v.w;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n_v += __shfl_xor(n_v, d, 64);
  } else if (tid < (int)(sizeof(RowState) / 4)) {
    reinterpret_cast<unsigned*>(&cur)[tid] = reinterpret_cast<const unsigned*>(st + row)[tid];
  }
  __syncthreads();
  if (init && tid == 0) {
    double t = 0.0;
    for (int q = 0; q < MT / 64; ++q) t += red[q];
    if (c == 0) counts[cl] = n_v;
    if (n_v >= 1) {
      const Ranks r = segment_ranks_of(n_v);
      cur.k[0] = cur.k[4] = (unsigned)r.m0;
      cur.k[1] = cur.k[5] = (unsigned)r.m1;
      cur.k[2] = (unsigned)r.l0;
      cur.k[3] = (unsigned)r.l1;
      __builtin_memcpy(cur.g, &r.g, 8);
    } else {                                                     // every histogram of the row stays empty: no lane finds a rank
      for (int q = 0; q < NSTATE; ++q) cur.k[q] = 0u;
    }
    const double rm = sqrt(t / (double)n_v);
    o[0] = (float)rm;
    o[4] = (float)(20.0 * log10(value_max / rm));               // +inf at rm == 0; NaN stays NaN
    cur.has_nan = ((t != t) ? 1u : 0u) | (n_v < 1 ? 2u : 0u);
  }
  if (init) __syncthreads();                                     // kernel-uniform: the ranks were written after the barrier above
  rank_scan(cur, cur.g, hrow, reps, group, pass, o, st + row);
}

bool sizes_ok(int n_cand, int n_classes, long long total) {
  return n_cand >= 1 && n_cand <= MAXC && n_classes >= 1 && n_classes <= MAXK && total > 0 && total < 0x100000000ll;
}

// ---- (b) slope classes ------------------------------------------------------------------------------------------------
struct Thresholds {
  float t[MAXT];
};

__global__ __launch_bounds__(256) void slope_classes_kernel(const float* __restrict__ z, long long pixels, const long long* __restrict__ scenes,
                                                           int n_scenes, Thresholds T, int n_thr, const unsigned char* __restrict__ valid,
                                                           unsigned char* __restrict__ out) {
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long long)gridDim.x * 256) {
    const long long* sc = scenes + (size_t)find_row(scenes, n_scenes, 3, 0, p) * 3;
    const long long off = sc[0], h = sc[1], w = sc[2];
    unsigned char label = 255;
    if (off >= 0 && h > 0 && w > 0 && h < 0x7fffffffll && w < 0x7fffffffll && p >= off && p - off < h * w && off + h * w <= pixels) {
      const long long local = p - off;
      const long long y = local < 0x100000000ll ? (long long)((unsigned)local / (unsigned)w) : local / w;   // the usual case: 32 bits
      const long long x = local - y * w;
      const long long ys[3] = {y > 0 ? y - 1 : 0, y, y < h - 1 ? y + 1 : h - 1};
      const long long xs[3] = {x > 0 ? x - 1 : 0, x, x < w - 1 ? x + 1 : w - 1};
      float t[3][3];
      bool ok = true;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const long long j = off + ys[r] * w + xs[q];             // inside [off, off + h w): inside the plane
          t[r][q] = z[j];
          if (valid != nullptr) ok = ok && valid[j] != 0;
        }
      // a b c / d e f / g h i
      const float a = t[0][0], b = t[0][1], c = t[0][2], d = t[1][0], f = t[1][2], g = t[2][0], hh = t[2][1], i = t[2][2];
      const float gx = __fsub_rn(__fadd_rn(__fadd_rn(c, __fmul_rn(2.f, f)), i), __fadd_rn(__fadd_rn(a, __fmul_rn(2.f, d)), g));
      const float gy = __fsub_rn(__fadd_rn(__fadd_rn(g, __fmul_rn(2.f, hh)), i), __fadd_rn(__fadd_rn(a, __fmul_rn(2.f, b)), c));
      const float pp = __fadd_rn(__fmul_rn(gx, gx), __fmul_rn(gy, gy));
      if (ok && pp == pp) {
        int n = 0;
        for (int k = 0; k < n_thr; ++k) n += T.t[k] <= pp ? 1 : 0;
        label = (unsigned char)n;
      }
    }
    out[p] = label;
  }
}

}  // namespace

extern "C" size_t jspsr_strata_workspace_bytes(int n_cand, int n_classes, long long total) {
  if (!sizes_ok(n_cand, n_classes, total)) return 0;
  const long long n_runs = (total + RUN - 1) / RUN;
  const size_t rows = (size_t)n_cand * n_classes;
  return up16((size_t)n_cand * total * sizeof(float)) + up16((size_t)n_cand * n_runs * n_classes * sizeof(double)) +
         rows * hist_replicas(rows, n_runs) * NSTATE * 256 * sizeof(unsigned) + rows * sizeof(RowState) + 64 + up16((size_t)total);
}

extern "C" int jspsr_strata_forward(const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                                    long long gt_numel, const unsigned char* labels, long long labels_numel, int n_classes,
                                    const unsigned char* valid, long long valid_numel, const long long* windows, int n_windows,
                                    long long total, double value_max, float* out, long long* counts, void* workspace,
                                    jspsr_stream_t stream) {
  const char* const name = "strata_forward";
  if (n_cand < 1 || n_cand > MAXC) return fail(JSPSR_EINVAL, "%s: n_cand = %d is outside 1..%d", name, n_cand, MAXC);
  if (n_classes < 1 || n_classes > MAXK) return fail(JSPSR_EINVAL, "%s: n_classes = %d is outside 1..%d", name, n_classes, MAXK);
  if (!cands || !cand_numel || !gt || !labels || !windows || !out || !counts || !workspace) return fail(JSPSR_EINVAL, "%s: null pointer", name);
  if (n_windows <= 0 || total <= 0 || gt_numel <= 0) return fail(JSPSR_EINVAL, "%s: empty window table", name);
  if (labels_numel != gt_numel)
    return fail(JSPSR_EINVAL, "%s: the label plane has %lld elements, the ground truth %lld", name, labels_numel, gt_numel);
  if (valid && valid_numel != gt_numel)
    return fail(JSPSR_EINVAL, "%s: the validity plane has %lld elements, the ground truth %lld", name, valid_numel, gt_numel);
  if (total >= 0x100000000ll) return fail(JSPSR_EINVAL, "%s: %lld pooled elements, the rank counters hold fewer than 2^32", name, total);
  Buffers B;
  if (int err = pack_buffers(name, cands, cand_numel, n_cand, gt, gt_numel, B)) return err;
  if (!aligned4(gt) || !aligned4(out)) return fail(JSPSR_EALIGN, "%s: tensors not 4-byte aligned", name);
  if (reinterpret_cast<uintptr_t>(counts) & 7u) return fail(JSPSR_EALIGN, "%s: counts not 8-byte aligned", name);
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "%s: workspace not 16-byte aligned", name);
  const long long n_runs = (total + RUN - 1) / RUN;
  const size_t rows = (size_t)n_cand * n_classes;
  const int reps = hist_replicas(rows, n_runs);
  char* ws = static_cast<char*>(workspace);
  float* e = reinterpret_cast<float*>(ws);
  size_t off = up16((size_t)n_cand * total * sizeof(float));
  double* partial = reinterpret_cast<double*>(ws + off);
  off += up16((size_t)n_cand * n_runs * n_classes * sizeof(double));
  unsigned* hist = reinterpret_cast<unsigned*>(ws + off);
  const size_t hist_bytes = rows * reps * NSTATE * 256 * sizeof(unsigned);
  off += hist_bytes;
  RowState* st = reinterpret_cast<RowState*>(ws + off);
  unsigned char* cls = reinterpret_cast<unsigned char*>(ws + off + rows * sizeof(RowState) + 64);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the LDS of a workgroup grows with n_classes: up to 128 KiB, above the 64 KiB a kernel may take without asking
  const int lds_prepare = n_classes * (MT * (int)sizeof(double) + 512 * (int)sizeof(unsigned));
  const int lds_select[2] = {n_classes * 4 * 256 * (int)sizeof(unsigned), n_classes * 2 * 256 * (int)sizeof(unsigned)};
  static bool attr_set = false;
  if (!attr_set) {
    constexpr int lds_max = MAXK * 4 * 256 * (int)sizeof(unsigned);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(strata_prepare_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(strata_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess)
      return fail(JSPSR_EINVAL, "%s: raising the dynamic LDS limit failed: %s", name, hipGetErrorString(hipGetLastError()));
    attr_set = true;
  }
  if (hipMemsetAsync(hist, 0, hist_bytes, s) != hipSuccess)
    return fail(JSPSR_EINVAL, "%s: clearing the histograms failed: %s", name, hipGetErrorString(hipGetLastError()));
  const dim3 grid((unsigned)n_runs, n_cand);
  hipLaunchKernelGGL(strata_prepare_kernel, grid, dim3(MT), lds_prepare, s, B, labels, valid, windows, n_windows, total, n_runs, n_classes,
                     reps, e, cls, partial, hist);
  if (int err = check_launch("strata_prepare")) return err;
  for (int group = 0; group < 2; ++group) {
    for (int pass = 3; pass >= 0; --pass) {
      const int init = group == 0 && pass == 3;                  // the top digit of e and |e| was counted by the first pass
      if (!init) {
        hipLaunchKernelGGL(strata_select_kernel, grid, dim3(MT), lds_select[group], s, e, cls, total, n_classes, reps, group, pass, st, hist);
        if (int err = check_launch("strata_select")) return err;
      }
      hipLaunchKernelGGL(strata_scan_kernel, dim3((unsigned)rows), dim3(MT), 0, s, partial, n_runs, n_classes, reps, group, pass, init,
                         value_max, st, hist, out, counts);
      if (int err = check_launch("strata_select")) return err;   // the scans count as selects, as in K12
    }
  }
  return JSPSR_OK;
}

extern "C" int jspsr_slope_classes(const float* z, long long pixels, const long long* scenes, int n_scenes, const float* thresholds,
                                   int n_thr, const unsigned char* valid, long long valid_numel, unsigned char* out,
                                   jspsr_stream_t stream) {
  const char* const name = "slope_classes";
  if (!z || !scenes || !out || pixels <= 0 || n_scenes <= 0) return fail(JSPSR_EINVAL, "%s: null pointer or empty plane", name);
  if (n_thr < 0 || n_thr > MAXT || (n_thr > 0 && !thresholds)) return fail(JSPSR_EINVAL, "%s: n_thr = %d is outside 0..%d", name, n_thr, MAXT);
  if (valid && valid_numel != pixels)
    return fail(JSPSR_EINVAL, "%s: the validity plane has %lld elements, the rasters %lld", name, valid_numel, pixels);
  if (!aligned4(z)) return fail(JSPSR_EALIGN, "%s: rasters not 4-byte aligned", name);
  Thresholds T;
  for (int k = 0; k < MAXT; ++k) T.t[k] = k < n_thr ? thresholds[k] : 0.f;
  for (int k = 0; k < n_thr; ++k)
    if (!(T.t[k] >= 0.f) || (k > 0 && !(T.t[k] >= T.t[k - 1]))) return fail(JSPSR_EINVAL, "%s: thresholds must be >= 0 and ascending", name);
  long long blocks = (pixels + 255) / 256;
  blocks = blocks > 65536 ? 65536 : blocks;
  hipLaunchKernelGGL(slope_classes_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), z, pixels, scenes, n_scenes,
                     T, n_thr, valid, out);
  return check_launch("slope_classes");
}
