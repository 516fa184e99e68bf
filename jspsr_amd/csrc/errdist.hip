// K21 -- the whole-set error distribution on the device: the numbers behind the reference's figure "Elevation Error
// Distribution in [-5, 5] m" (summarise_evaluation, utils/utils.py:1394-1456).  For every candidate the reference takes
// the pooled errors e = dem - gt, keeps lo <= e <= hi, stores them as float16 and draws sns.kdeplot(bw_adjust=1, cut=0.5,
// common_norm=False): a Gaussian kernel density estimate with Scott's bandwidth on 200 points.  After the filter a float16
// takes one of K values (35 330 for [-5, 5]), so the whole input of the estimate is an integer histogram of K bins, and a
// Gaussian KDE over n points with repeated values is the same sum over the distinct values weighted by their counts.
// (a) jspsr_errdist_hist_forward: ONE launch.  Candidate c is walked by gridDim.x workgroups (blockIdx.y = c), the grid
//     sized so that all candidates together fill the chip once; a workgroup owns one contiguous range of the pooled
//     elements, read through the window table by csrc/pooled_read.h's pooled_fetch (a bisection when the window changes,
//     a 32-bit division on the usual path), and counts them into an
//     LDS image of up to LDS_BINS bins (147 456 B of dynamic LDS, raised with hipFuncSetAttribute: one workgroup per CU, 16
//     waves to hide the reads; it cannot be double-buffered).  A range with more bins than one image holds is walked once
//     per image of LDS_BINS bins (at most twice: float16 has 63 488 finite values), inside the same launch.  The image is
//     flushed with one 64-bit global add per occupied bin.  Integer adds only: a histogram has the same bits whatever
//     candidates share the call, whatever the grid is, on every run.
//     Contention: a baseline that equals the ground truth over water puts most of a wave's 64 increments into the two
//     bins of 0, a good model's errors spread over thousands of bins.  hist_add<ROUNDS, true> (summary_select.h) takes up
//     to ROUNDS (2) times the bin of the first pending lane, counts its lanes with a ballot and lets that lane add the
//     count once, the leader's bin by v_readlane; what is left adds one by one.  JSPSR_ERRDIST_ROUNDS = 0 / 1 / 2
//     selects the instance, for measurements only (profiles/r22_error_distribution_bench.txt).
// (b) jspsr_errdist_kde_forward: two launches, fp64.  stats: a workgroup per candidate folds n, the mean, the variance
//     (ddof 1, about the mean), Scott's bandwidth and numpy's linspace over the occupied support; density: a workgroup per
//     grid point and candidate sums count * exp(-(g - v)^2 / (2 bw^2)) over the occupied bins.  Every sum is folded per
//     thread over bins tid, tid + 256, ... and then by a fixed tree: the order depends on K alone.
// The float16 rounding, the key and the classification are __host__ __device__ integer code, so jspsr_errdist_key is the
// kernel's own arithmetic and the wave's FP16 denormal mode cannot matter.  Built with -ffp-contract=off: linspace is
// start + i * step with two roundings, as numpy forms it.
#include "common.h"
#include "pooled_read.h"
#include "summary_select.h"

#include <cmath>
#include <cstdlib>

namespace {

using namespace jspsr;

constexpr int HT = 1024;                      // threads of a histogram workgroup: 16 waves on the one CU its LDS image fills
constexpr int UNROLL = 4;
constexpr int STEP = HT * UNROLL;
constexpr int LDS_BINS = 36864;               // bins of one LDS image: 147 456 B (the default range needs 35 330)
constexpr int N_CU = 256;                     // MI355X
constexpr int KT = 256;                       // threads of the curve kernels
constexpr int WS_WORDS = 8;                   // doubles per candidate between the two curve kernels

// float32 bits -> float16 bits: round to nearest, ties to even, subnormals produced; np.float32(x).astype(np.float16).
__host__ __device__ inline unsigned f16_bits(unsigned u) {
  const unsigned sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | 0x7e00u;                    // NaN
  if (a >= 0x477ff000u) return sign | 0x7c00u;                   // >= 65520 rounds to inf
  if (a >= 0x38800000u) {                                        // a normal float16: re-bias, round the 13 dropped bits
    const unsigned r = a - 0x38000000u;
    return sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13);       // a carry out of the mantissa raises the exponent
  }
  const unsigned e = a >> 23;
  if (e < 102u) return sign;                                     // below 2^-25: zero
  const unsigned m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;   // units of 2^-24; shift in 14 .. 24
  unsigned r = m >> shift;
  const unsigned rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
  if (rem > half || (rem == half && (r & 1u))) ++r;              // r = 1024 is the smallest normal
  return sign | r;
}
__host__ __device__ inline int f16_key(unsigned bits) { return (int)(bits ^ ((bits & 0x8000u) ? 0xffffu : 0x8000u)); }
__host__ __device__ inline unsigned f32_bits(float f) {
  unsigned u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
__host__ __device__ inline double f16_value(unsigned bits) {    // exact
  const unsigned ex = (bits >> 10) & 31u, m = bits & 1023u;
  const double v = ex ? ldexp((double)(1024u + m), (int)ex - 25) : ldexp((double)m, -24);
  return (bits & 0x8000u) ? -v : v;
}
__host__ __device__ inline double bin_value(int key0, int b) {
  const unsigned k = (unsigned)(key0 + b);
  return f16_value((k & 0x8000u) ? (k ^ 0x8000u) : (k ^ 0xffffu));
}

struct Range {
  float lo, hi;
  int key0, K;
};
bool make_range(double lo, double hi, Range& r) {
  if (!(lo <= hi) || !(fabs(lo) <= 65504.0) || !(fabs(hi) <= 65504.0)) return false;      // NaN fails every comparison
  r.lo = (float)lo;
  r.hi = (float)hi;
  r.key0 = f16_key(f16_bits(f32_bits(r.lo)));
  r.K = f16_key(f16_bits(f32_bits(r.hi))) - r.key0 + 1;
  return true;
}
// The bin of a scored error, or -1 below the range, -2 above it, -3 a NaN.  lo = +0 keeps e = -0 (the comparison says so)
// although -0's key lies one below key0; it is counted with +0, the same value (the clamp; no other element can leave [0, K):
// the rounding is monotone).
__host__ __device__ inline int classify(float e, const Range& r) {
  if (e >= r.lo && e <= r.hi) {
    const int b = f16_key(f16_bits(f32_bits(e))) - r.key0;
    return b < 0 ? 0 : (b >= r.K ? r.K - 1 : b);
  }
  return e < r.lo ? -1 : (e > r.hi ? -2 : -3);
}

template <bool MASKED, int ROUNDS>
__global__ __launch_bounds__(HT) void errdist_hist_kernel(Buffers B, const unsigned char* __restrict__ plane, const long long* __restrict__ win,
                                                         int n_win, long long total, long long per_wg, Range R,
                                                         unsigned long long* __restrict__ hist, unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned image[];                            // LDS_BINS counters
  __shared__ unsigned wred[4][HT / 64];
  const int tid = threadIdx.x, c = blockIdx.y;
  const long long lo = (long long)blockIdx.x * per_wg;
  const long long hi = lo + per_wg < total ? lo + per_wg : total;
  if (lo >= hi) return;                                          // workgroup-uniform
  unsigned n_scored = 0u, n_in = 0u, n_below = 0u, n_above = 0u;   // this thread's; fewer than 2^32 elements per call
  for (int first = 0; first < R.K; first += LDS_BINS) {          // one walk per image; kernel-uniform
    const int bins = R.K - first < LDS_BINS ? R.K - first : LDS_BINS;
    for (int b = tid; b < bins; b += HT) image[b] = 0u;
    __syncthreads();
    WindowCursor W(B, c);
    for (long long base = lo; base < hi; base += STEP) {
      int bin[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const long long p = base + u * HT + tid;
        bin[u] = -4;                                             // not scored
        if (p >= hi) continue;
        float v;                                                 // a NaN, scored: an element no window covers, or a read outside a buffer
        bool keep = true;
        pooled_fetch(W, win, n_win, p, v, [&](long long jg) {
          if constexpr (MASKED) keep = plane[jg] != 0;            // the plane has gt's numel (checked by the entry)
        });
        if (keep) bin[u] = classify(v, R);                        // a masked element's v is looked at nowhere
      }
      if (first == 0) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
          n_scored += bin[u] != -4 ? 1u : 0u;
          n_in += bin[u] >= 0 ? 1u : 0u;
          n_below += bin[u] == -1 ? 1u : 0u;
          n_above += bin[u] == -2 ? 1u : 0u;
        }
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const int b = bin[u] - first;
        hist_add<ROUNDS, true>(image, bin[u] >= 0 && b >= 0 && b < bins, (unsigned)b);
      }
    }
    __syncthreads();
    unsigned long long* __restrict__ out = hist + (size_t)c * R.K + first;
    for (int b = tid; b < bins; b += HT) {
      const unsigned v = image[b];
      if (v) atomicAdd(&out[b], (unsigned long long)v);
    }
    __syncthreads();                                             // the image is cleared again for the next range of bins
  }
  unsigned cnt[4] = {n_scored, n_in, n_below, n_above};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt[k] += (unsigned)__shfl_xor((int)cnt[k], d, 64);    // at most 64 * 2^26: no overflow below 2^32 elements
    if ((tid & 63) == 0) wred[k][tid >> 6] = cnt[k];
  }
  __syncthreads();
  if (tid < 4) {
    unsigned long long t = 0ull;
    for (int q = 0; q < HT / 64; ++q) t += wred[tid][q];
    if (t) atomicAdd(&counts[(size_t)c * 4 + tid], t);
  }
}

// ---- (b) the curve -------------------------------------------------------------------------------------------------
// fold red[0 .. KT) into red[0] by a fixed tree; every thread of the workgroup arrives
__device__ __forceinline__ double tree_sum(double* red, double v) {
  const int tid = threadIdx.x;
  __syncthreads();                                               // red may still be read from the fold before
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int d = KT / 2; d > 0; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  return red[0];
}

// ws[c] = { n, mean, bw, 0 .. }; stats[c] = { mean, std, bw }; support[c][j]
__global__ __launch_bounds__(KT) void errdist_stats_kernel(const long long* __restrict__ hist, int key0, int K, int gridsize, double cut,
                                                          double bw_adjust, double* __restrict__ support, double* __restrict__ stats,
                                                          double* __restrict__ ws) {
  __shared__ double red[KT], lin[3];
  __shared__ int bmin[KT], bmax[KT];
  const int tid = threadIdx.x, c = blockIdx.x;
  const long long* __restrict__ h = hist + (size_t)c * K;
  double n_t = 0.0, s1 = 0.0;                                    // counts below 2^32 each, their sum below 2^53: exact in double
  int lo_b = K, hi_b = -1;
  for (int b = tid; b < K; b += KT) {
    const long long cnt = h[b];
    if (cnt <= 0) continue;
    n_t += (double)cnt;
    s1 += (double)cnt * bin_value(key0, b);
    lo_b = b < lo_b ? b : lo_b;
    hi_b = b;
  }
  const double n = tree_sum(red, n_t);
  const double mean = tree_sum(red, s1) / n;                     // n = 0: NaN
  bmin[tid] = lo_b;
  bmax[tid] = hi_b;
  double ss = 0.0;
  for (int b = tid; b < K; b += KT) {
    const long long cnt = h[b];
    if (cnt <= 0) continue;
    const double d = bin_value(key0, b) - mean;
    ss += (double)cnt * (d * d);
  }
  const double var = tree_sum(red, ss) / (n - 1.0);              // n = 1: 0 / 0, NaN
  if (tid == 0) {
    int b0 = K, b1 = -1;
    for (int q = 0; q < KT; ++q) {
      b0 = bmin[q] < b0 ? bmin[q] : b0;
      b1 = bmax[q] > b1 ? bmax[q] : b1;
    }
    const double nanv = __builtin_nan("");
    const bool ok = n >= 2.0 && var > 0.0;                       // a NaN variance fails
    const double sd = n >= 2.0 ? sqrt(var) : nanv;
    const double bw = n >= 2.0 ? sd * pow(n, -0.2) * bw_adjust : nanv;
    stats[c * 3 + 0] = mean;
    stats[c * 3 + 1] = sd;
    stats[c * 3 + 2] = bw;
    double start = nanv, stop = nanv, step = nanv;
    if (ok) {
      start = bin_value(key0, b0) - cut * bw;
      stop = bin_value(key0, b1) + cut * bw;
      step = (stop - start) / (double)(gridsize - 1);
    }
    ws[c * WS_WORDS + 0] = n;
    ws[c * WS_WORDS + 1] = ok ? bw : nanv;
    lin[0] = start;
    lin[1] = stop;
    lin[2] = step;
  }
  __syncthreads();
  const double start = lin[0], stop = lin[1], step = lin[2];
  for (int j = tid; j < gridsize; j += KT) {                     // numpy.linspace: arange * step + start, the last point is stop
    const double g = step != 0.0 ? (double)j * step + start : (double)j * (stop - start) + start;
    support[(size_t)c * gridsize + j] = j == gridsize - 1 ? stop : g;
  }
}

__global__ __launch_bounds__(KT) void errdist_density_kernel(const long long* __restrict__ hist, int key0, int K, int gridsize,
                                                            const double* __restrict__ support, const double* __restrict__ ws,
                                                            double* __restrict__ density) {
  __shared__ double red[KT];
  const int tid = threadIdx.x, j = blockIdx.x, c = blockIdx.y;
  const double n = ws[c * WS_WORDS + 0], bw = ws[c * WS_WORDS + 1];
  double* o = density + (size_t)c * gridsize + j;
  if (!(bw > 0.0)) {                                             // workgroup-uniform: n < 2 or no variance
    if (tid == 0) *o = __builtin_nan("");
    return;
  }
  const long long* __restrict__ h = hist + (size_t)c * K;
  const double g = support[(size_t)c * gridsize + j], two_bw2 = 2.0 * (bw * bw);
  double acc = 0.0;
  for (int b = tid; b < K; b += KT) {
    const long long cnt = h[b];
    if (cnt <= 0) continue;
    const double d = g - bin_value(key0, b);
    acc += (double)cnt * exp(-(d * d) / two_bw2);
  }
  const double sum = tree_sum(red, acc);
  if (tid == 0) *o = sum / (n * bw * 2.5066282746310002);        // sqrt(2 pi)
}

template <bool MASKED>
void launch_hist(int rounds, dim3 grid, hipStream_t s, const Buffers& B, const unsigned char* plane, const long long* win, int n_win,
                 long long total, long long per_wg, const Range& R, unsigned long long* hist, unsigned long long* counts) {
  constexpr int lds = LDS_BINS * (int)sizeof(unsigned);
#define JSPSR_ERRDIST_LAUNCH(RN)                                                                                                   \
  {                                                                                                                                \
    static bool attr_set = false;                                                                                                  \
    if (!attr_set) {                                                                                                               \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(errdist_hist_kernel<MASKED, RN>),                                   \
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds);                                                  \
      attr_set = true;                                                                                                             \
    }                                                                                                                              \
    hipLaunchKernelGGL((errdist_hist_kernel<MASKED, RN>), grid, dim3(HT), lds, s, B, plane, win, n_win, total, per_wg, R, hist,   \
                       counts);                                                                                                    \
  }
  if (rounds == 0) JSPSR_ERRDIST_LAUNCH(0)
  else if (rounds == 1) JSPSR_ERRDIST_LAUNCH(1)
  else JSPSR_ERRDIST_LAUNCH(2)
#undef JSPSR_ERRDIST_LAUNCH
}

}  // namespace

extern "C" int jspsr_errdist_bins(double lo, double hi, int* key0, int* K) {
  Range r;
  if (!key0 || !K) return fail(JSPSR_EINVAL, "errdist_bins: null pointer");
  if (!make_range(lo, hi, r)) return fail(JSPSR_EINVAL, "errdist_bins: lo = %g, hi = %g (lo <= hi, both finite, magnitudes <= 65504)", lo, hi);
  *key0 = r.key0;
  *K = r.K;
  return JSPSR_OK;
}

extern "C" int jspsr_errdist_key(float e, double lo, double hi) {
  Range r;
  if (!make_range(lo, hi, r)) {
    fail(JSPSR_EINVAL, "errdist_key: lo = %g, hi = %g (lo <= hi, both finite, magnitudes <= 65504)", lo, hi);
    return -4;
  }
  return classify(e, r);
}

extern "C" size_t jspsr_errdist_workspace_bytes(int n_cand, int gridsize) {
  if (n_cand < 1 || n_cand > MAXC || gridsize < 2 || gridsize > 65535) return 0;     // the entry's own bounds
  return (size_t)n_cand * WS_WORDS * sizeof(double);
}

extern "C" int jspsr_errdist_hist_forward(const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                                          long long gt_numel, const unsigned char* valid, long long valid_numel,
                                          const long long* windows, int n_windows, long long total, double lo, double hi,
                                          long long* hist, long long* counts, jspsr_stream_t stream) {
  const char* const name = "errdist_hist_forward";
  if (n_cand < 1 || n_cand > MAXC) return fail(JSPSR_EINVAL, "%s: n_cand = %d is outside 1..%d", name, n_cand, MAXC);
  if (!cands || !cand_numel || !gt || !windows || !hist || !counts) return fail(JSPSR_EINVAL, "%s: null pointer", name);
  if (n_windows <= 0 || total <= 0 || gt_numel <= 0) return fail(JSPSR_EINVAL, "%s: empty window table", name);
  if (valid && valid_numel != gt_numel)
    return fail(JSPSR_EINVAL, "%s: the validity plane has %lld elements, the ground truth %lld", name, valid_numel, gt_numel);
  if (total >= 0x100000000ll) return fail(JSPSR_EINVAL, "%s: %lld pooled elements, the bin counters hold fewer than 2^32", name, total);
  Range R;
  if (!make_range(lo, hi, R)) return fail(JSPSR_EINVAL, "%s: lo = %g, hi = %g (lo <= hi, both finite, magnitudes <= 65504)", name, lo, hi);
  Buffers B;
  if (int err = pack_buffers(name, cands, cand_numel, n_cand, gt, gt_numel, B)) return err;
  if (!aligned4(gt)) return fail(JSPSR_EALIGN, "%s: ground truth not 4-byte aligned", name);
  if ((reinterpret_cast<uintptr_t>(hist) & 7u) || (reinterpret_cast<uintptr_t>(counts) & 7u))
    return fail(JSPSR_EALIGN, "%s: hist and counts must be 8-byte aligned", name);
  static const int rounds = [] { const char* e = getenv("JSPSR_ERRDIST_ROUNDS"); const int r = e ? atoi(e) : 2; return r < 0 ? 0 : (r > 2 ? 2 : r); }();
  hipStream_t s = static_cast<hipStream_t>(stream);
  // hist and counts are adjacent in no way the caller promises: two clears
  if (hipMemsetAsync(hist, 0, (size_t)n_cand * R.K * sizeof(long long), s) != hipSuccess ||
      hipMemsetAsync(counts, 0, (size_t)n_cand * 4 * sizeof(long long), s) != hipSuccess)
    return fail(JSPSR_EINVAL, "%s: clearing the histograms failed: %s", name, hipGetErrorString(hipGetLastError()));
  // all candidates together fill the chip once; a workgroup owns a whole number of unrolled steps
  long long wgs = N_CU / n_cand;
  const long long steps = (total + STEP - 1) / STEP;
  wgs = wgs > steps ? steps : wgs;
  const long long per_wg = (steps + wgs - 1) / wgs * STEP;
  wgs = (total + per_wg - 1) / per_wg;
  const dim3 grid((unsigned)wgs, n_cand);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  unsigned long long* n = reinterpret_cast<unsigned long long*>(counts);
  if (valid) launch_hist<true>(rounds, grid, s, B, valid, windows, n_windows, total, per_wg, R, h, n);
  else launch_hist<false>(rounds, grid, s, B, nullptr, windows, n_windows, total, per_wg, R, h, n);
  return check_launch(valid ? "errdist_hist (valid)" : "errdist_hist");
}

extern "C" int jspsr_errdist_kde_forward(const long long* hist, int n_cand, int key0, int K, int gridsize, double cut, double bw_adjust,
                                         double* support, double* density, double* stats, void* workspace, jspsr_stream_t stream) {
  const char* const name = "errdist_kde_forward";
  if (n_cand < 1 || n_cand > MAXC) return fail(JSPSR_EINVAL, "%s: n_cand = %d is outside 1..%d", name, n_cand, MAXC);
  if (!hist || !support || !density || !stats || !workspace) return fail(JSPSR_EINVAL, "%s: null pointer", name);
  if (K < 1 || key0 < 0x0400 || key0 + K - 1 > 0xfbff)           // the keys of -65504 and 65504
    return fail(JSPSR_EINVAL, "%s: key0 = %d, K = %d are not bins of finite float16 values", name, key0, K);
  if (gridsize < 2 || gridsize > 65535) return fail(JSPSR_EINVAL, "%s: gridsize = %d is outside 2..65535", name, gridsize);
  if (!(cut >= 0.0) || !(bw_adjust > 0.0) || !std::isfinite(cut) || !std::isfinite(bw_adjust))
    return fail(JSPSR_EINVAL, "%s: cut = %g, bw_adjust = %g (cut >= 0, bw_adjust > 0, both finite)", name, cut, bw_adjust);
  if ((reinterpret_cast<uintptr_t>(hist) & 7u) || (reinterpret_cast<uintptr_t>(support) & 7u) || (reinterpret_cast<uintptr_t>(density) & 7u) ||
      (reinterpret_cast<uintptr_t>(stats) & 7u))
    return fail(JSPSR_EALIGN, "%s: tensors not 8-byte aligned", name);
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "%s: workspace not 16-byte aligned", name);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* ws = static_cast<double*>(workspace);
  hipLaunchKernelGGL(errdist_stats_kernel, dim3(n_cand), dim3(KT), 0, s, hist, key0, K, gridsize, cut, bw_adjust, support, stats, ws);
  if (int err = check_launch("errdist_kde")) return err;
  hipLaunchKernelGGL(errdist_density_kernel, dim3(gridsize, n_cand), dim3(KT), 0, s, hist, key0, K, gridsize, support, ws, density);
  return check_launch("errdist_kde");
}
