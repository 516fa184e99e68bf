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
//       scan      a workgroup per (candidate, class), K18's scan.  The class count n_c is the sum of the class's top-digit
//                 histogram of e (integers, exact), so the ranks, the LE95 weight and the divisor of the sum are formed
//                 there by segment_ranks_of (summary_select.h), the inline K18 uses.
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
#include "summary_select.h"

#include <cmath>

namespace {

using namespace jspsr;

constexpr int MT = 256;
constexpr int UNROLL = 4;
constexpr int RUN = 8192;                     // pooled elements per workgroup and per fp64 partial sum (jspsr_amd/summary.py: CHUNK)
constexpr int NSTATE = 6;                     // ranks: median lo, hi | LE95 lo, hi | MAD lo, hi
constexpr int NOUT = 11;
constexpr int MAXC = 8;
constexpr int MAXK = 32;                      // classes
constexpr int NONE = 255;                     // the class byte of an element that belongs to no class
constexpr int WIN_WORDS = 4 + 2 * (1 + MAXC); // K12's window row: segment (not read), h, w, e offset, {offset, pitch} of gt, cand 0..7
constexpr int MAXT = 31;                      // slope thresholds
static_assert(RUN % (MT * UNROLL) == 0, "a run is a whole number of unrolled steps");

struct RowState {            // one per (candidate, class), in device memory; 64 bytes (csrc/summary.hip's)
  unsigned prefix[NSTATE];   // key bits fixed so far (high bits)
  unsigned k[NSTATE];        // rank still to find inside the current prefix class (0-based)
  float center;              // the median, for |e - median|
  unsigned has_nan;          // bit 0: the fp64 sum is NaN; bit 1: the class is empty
  unsigned g[2];             // the bits of the LE95 weight
};
static_assert(sizeof(RowState) == 64, "RowState layout");

struct Buffers {             // by value in the kernel arguments
  const float* cand[MAXC];
  long long cand_numel[MAXC];
  const float* gt;
  long long gt_numel;
  const unsigned char* labels;   // gt's layout and numel
  const unsigned char* valid;    // gt's layout and numel, or null
};

// LDS of prepare: n_classes x { 2 x 256 counters, 256 doubles }; of select: n_classes x slots x 256 counters
__global__ __launch_bounds__(MT) void strata_prepare_kernel(Buffers B, const long long* __restrict__ win, int n_win, long long total,
                                                           long long n_runs, int n_classes, int reps, float* __restrict__ e_all,
                                                           unsigned char* __restrict__ cls_all, double* __restrict__ partial,
                                                           unsigned* __restrict__ hist) {
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
  const float* __restrict__ cp = B.cand[c];
  const float* __restrict__ gp = B.gt;
  const long long cn = B.cand_numel[c], gn = B.gt_numel;
  float* __restrict__ e = e_all + (size_t)c * total;
  long long w_lo = 0, w_hi = 0, w_w = 1, goff = 0, gpitch = 0, coff = 0, cpitch = 0;   // the window of the last element
  bool w_ok = false;
  for (long long base = lo; base < hi; base += MT * UNROLL) {
    float err[UNROLL];
    int cls[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long long p = base + u * MT + tid;
      cls[u] = NONE;
      err[u] = 0.f;
      if (p >= hi) continue;
      if (p < w_lo || p >= w_hi) {
        const long long* wr = win + (size_t)find_row(win, n_win, WIN_WORDS, 3, p) * WIN_WORDS;
        w_w = wr[2];
        w_lo = wr[3];
        w_hi = w_lo + wr[1] * w_w;
        w_ok = wr[1] > 0 && w_w > 0;
        goff = wr[4]; gpitch = wr[5];
        coff = wr[6 + 2 * c]; cpitch = wr[7 + 2 * c];
      }
      float v = __builtin_nanf("");                             // an element no window covers, or a read outside a buffer:
      int k = 0;                                                // a NaN of class 0, so that a bad table shows (K12 does the same)
      if (w_ok && p >= w_lo && p < w_hi) {
        const long long local = p - w_lo;
        long long y;
        if (local < 0x100000000ll && w_w < 0x100000000ll) y = (long long)((unsigned)local / (unsigned)w_w);   // the usual case
        else y = local / w_w;
        const long long x = local - y * w_w;
        const long long jc = coff + y * cpitch + x, jg = goff + y * gpitch + x;
        if (jc >= 0 && jc < cn && jg >= 0 && jg < gn) {
          v = __fsub_rn(cp[jc], gp[jg]);
          k = B.labels[jg];                                       // the planes have gt's numel (checked by the entry)
          if (k >= n_classes) k = NONE;
          if (B.valid != nullptr && B.valid[jg] == 0) k = NONE;
        }
      }
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

// One workgroup per (candidate, class), a wave per state: csrc/summary.hip's masked scan with the count taken from the
// class's top-digit histogram of e.  init: the first scan of a call -- n_c, the ranks, RMSE / PSNR from the run sums.
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
  // a wave per state
  const int q = (group ? 4 : 0) + wave, ql = q & ~1;
  const bool active = group ? wave < 2 : true;
  const int shift = pass * 8;
  const unsigned himask = pass == 3 ? 0u : (0xffffffffu << (shift + 8));
  unsigned new_prefix = 0u, new_k = 0u;
  bool found = false;
  if (active) {
    const unsigned prefix = cur.prefix[q], k = cur.k[q];
    const bool same = ((prefix ^ cur.prefix[ql]) & himask) == 0u;       // counted once, under the pair's lower state
    const unsigned* h = hrow + (same ? ql : q) * 256 + 4 * lane;         // lane l owns bins 4l .. 4l+3
    unsigned c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
    for (int r = 0; r < reps; ++r) {
      const uint4 v = *reinterpret_cast<const uint4*>(h + (size_t)r * NSTATE * 256);
      c0 += v.x; c1 += v.y; c2 += v.z; c3 += v.w;
    }
    const unsigned own = c0 + c1 + c2 + c3;
    unsigned incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl += up;
    }
    const unsigned excl = incl - own;
    if (k >= excl && k < incl) {                                 // exactly one lane: the counts sum to more than k (none: an empty class)
      unsigned run = excl;
      int b = 0;
      if (k >= run + c0) { run += c0; b = 1;
        if (k >= run + c1) { run += c1; b = 2;
          if (k >= run + c2) { run += c2; b = 3; } } }
      new_k = k - run;
      new_prefix = prefix | ((unsigned)(4 * lane + b) << shift);
      found = true;
    }
  }
  __syncthreads();                                               // every wave has read the states and its histogram
  if (found) { cur.prefix[q] = new_prefix; cur.k[q] = new_k; }
  {                                                              // clear what this group's passes count into: states 0..3 or 4, 5
    const int first = group ? 4 : 0, quads = (group ? 2 : 4) * 64; // uint4 per replica
    for (int i = tid; i < reps * quads; i += MT)
      reinterpret_cast<uint4*>(hrow + ((size_t)(i / quads) * NSTATE + first) * 256)[i % quads] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  if (pass == 0 && tid == 0) {
    const float nanv = __builtin_nanf("");
    const bool bad = cur.has_nan != 0u, empty = (cur.has_nan & 2u) != 0u;
    if (!group) {
      const float m0 = key_value(cur.prefix[0]), m1 = key_value(cur.prefix[1]);
      const float l0 = key_value(cur.prefix[2]), l1 = key_value(cur.prefix[3]);
      const float med = __fmul_rn(__fadd_rn(m0, m1), 0.5f);      // np.median of a float32 array: mean of the two middle elements
      double g;
      __builtin_memcpy(&g, cur.g, 8);
      const float le = (float)((double)l0 + ((double)l1 - (double)l0) * g);
      cur.center = med;
      o[1] = bad ? nanv : med;
      o[3] = bad ? nanv : le;
      o[5] = empty ? nanv : m0; o[6] = empty ? nanv : m1; o[9] = empty ? nanv : l0; o[10] = empty ? nanv : l1;
      if (bad) { o[0] = nanv; o[4] = nanv; }
    } else {
      const float d0 = key_value(cur.prefix[4]), d1 = key_value(cur.prefix[5]);
      const float mad = __fmul_rn(__fadd_rn(d0, d1), 0.5f);
      o[2] = bad ? nanv : (float)(1.4826 * (double)mad);
      o[7] = empty ? nanv : d0; o[8] = empty ? nanv : d1;
    }
  }
  __syncthreads();
  if (tid < (int)(sizeof(RowState) / 4)) reinterpret_cast<unsigned*>(st + row)[tid] = reinterpret_cast<const unsigned*>(&cur)[tid];
}

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// Replicas of a row's histograms (csrc/summary.hip: hist_replicas): run r adds to replica r % reps, the scan sums them.  A
// power of two, at most 16, one per 64 runs of the pool.
int hist_replicas(long long n_runs) {
  int r = 1;
  while (r < 16 && (long long)r * 64 < n_runs) r *= 2;
  return r;
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
         rows * hist_replicas(n_runs) * NSTATE * 256 * sizeof(unsigned) + rows * sizeof(RowState) + 64 + up16((size_t)total);
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
  for (int c = 0; c < MAXC; ++c) {
    B.cand[c] = c < n_cand ? cands[c] : nullptr;
    B.cand_numel[c] = c < n_cand ? cand_numel[c] : 0;
    if (c < n_cand && (!cands[c] || cand_numel[c] <= 0)) return fail(JSPSR_EINVAL, "%s: candidate %d is null or empty", name, c);
    if (c < n_cand && !aligned4(cands[c])) return fail(JSPSR_EALIGN, "%s: candidate %d not 4-byte aligned", name, c);
  }
  B.gt = gt;
  B.gt_numel = gt_numel;
  B.labels = labels;
  B.valid = valid;
  if (!aligned4(gt) || !aligned4(out)) return fail(JSPSR_EALIGN, "%s: tensors not 4-byte aligned", name);
  if (reinterpret_cast<uintptr_t>(counts) & 7u) return fail(JSPSR_EALIGN, "%s: counts not 8-byte aligned", name);
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "%s: workspace not 16-byte aligned", name);
  const long long n_runs = (total + RUN - 1) / RUN;
  const size_t rows = (size_t)n_cand * n_classes;
  const int reps = hist_replicas(n_runs);
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
  hipLaunchKernelGGL(strata_prepare_kernel, grid, dim3(MT), lds_prepare, s, B, windows, n_windows, total, n_runs, n_classes, reps, e, cls,
                     partial, hist);
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
