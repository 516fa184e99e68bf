// K12 -- the whole-set validation summary on the device: what the reference's --val path
// does on the host after the model has run, through GeoTIFF files and numpy:
//   * save_prediction_to_disk    evaluation/evaluate_utils.py:242-271   clip to [0,1], descale_data, + base
//   * merge_dem(copyto_add)      utils/utils.py:914-967 (called at :1272)   the feather merge of a scene's 9 / 4 tiles
//   * summarise_evaluation       utils/utils.py:1238-1356   RMSE, median, NMAD, LE95, PSNR of the errors of ALL scenes
//                                pooled, for the prediction and every baseline DEM against the ground truth
// (a) jspsr_scenes_assemble_f32: clamp, de-scale, + base and the feather merge of every scene of a batch in ONE launch,
//     each mosaic written at its own offset of one pooled buffer.  tiles_merge_kernel's loop (csrc/tiles.hip) over
//     to_metres, ramp_weight and feather_add, the statements K8 uses (scene_finish.h), rounded one by one (this file is
//     built with -ffp-contract=off): the bits of clamp -> descale_data -> + base -> merge_tiles run scene by scene.
// (b) jspsr_summary_forward: pooled scores of n_cand candidates against one ground truth over a table of pitched
//     windows grouped into segments.  A streaming selection:
//       prepare   reads the candidate and the ground truth through the window table (pooled_read.h: the reader K21 and
//                 K22 use too), writes e = cand - gt once (candidate-major, a segment's windows back to back), folds
//                 sum e^2 in double per CHUNK of a segment and counts the top digit of the keys of e and |e|;
//       select    8 bits per pass on the order-preserving keys of summary_select.h.  Both ranks of a statistic are
//                 carried as two states whose prefixes may diverge (while they agree, one histogram serves both); the
//                 median and the LE95 select share each read of e; the |e - median| select follows.
//     16 launches whatever the number of windows, segments and candidates is: prepare, 4 scans + 3 reads of e for the
//     median / LE95 digits, 4 + 4 for the MAD.  A workgroup owns one CHUNK of one segment, so every sum is folded in an
//     order that depends on the segment's own size only: a row has the same bits for every n_cand, for every set of
//     other segments in the call, on every run.  The workgroups of a row flush their LDS counts into one of up to 16
//     replicas of the row's counters (hist_replicas): global adds to one address serialise.  The scan kernel is its
//     own init block (where the count and the fp64 sum come from) in front of rank_scan (summary_select.h), the part
//     K22's scan shares: the rank search, the clear of the replicas, the scores, the state write-back.
// (c) jspsr_summary_valid_forward (K18): (b) over the elements a validity plane in the ground truth's layout keeps.  The
//     three kernels are templates on MASKED; the unmasked instances are (b) as it was.  prepare reads the plane through
//     the window table, keeps a validity byte per pooled element (written once, by the workgroups of candidate 0, read
//     by every select pass of every candidate), leaves masked elements out of the fp64 sum and of every histogram and
//     writes its chunk's count of valid elements.  With a mask the number of valid elements n_v of a segment is data on
//     the device: the first scan folds the chunk counts into n_v and forms the ranks, the LE95 weight (kept in the row
//     state) and the divisor of the sum from it (segment_ranks_of: one __host__ __device__ inline, the bits of
//     jspsr_amd/summary.py: segment_ranks).  Masked lanes arrive at hist_add with match = false, they do not branch
//     around it.  A workgroup still owns one CHUNK of one segment of the UNMASKED numbering, and masked elements add
//     nothing: an all-ones plane gives (b)'s bits.  n_v = 0: no lane of the scan finds the rank, the states stay
//     where they are, and the row is written as NaN.
// Departures from the reference (numpy on float32 arrays), see include/jspsr_hip.h: RMSE from an fp64 sum rounded once
// (not numpy's fp32 pairwise mean); LE95's virtual index in double (numpy 2 forms it in float32 for float32 input); PSNR
// without the 1e-8 the reference's online form adds for the baselines.
#include "common.h"
#include "pooled_read.h"
#include "scene_finish.h"
#include "summary_select.h"

#include <cmath>

namespace {

using namespace jspsr;

constexpr int MT = SCAN_MT;
constexpr int UNROLL = 4;
constexpr int CHUNK = 8192;                   // elements of a segment per workgroup (jspsr_amd/summary.py: CHUNK)
constexpr int SEG_WORDS = 8;                  // e start, n, first chunk, 4 ranks, g (fp64 bits)
static_assert(CHUNK % (MT * UNROLL) == 0, "a chunk is a whole number of unrolled steps");

// ---- (a) scene assembly --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scenes_assemble_kernel(const float* __restrict__ tiles, const float* __restrict__ base,
                                                             const float* __restrict__ ramp, float* __restrict__ out,
                                                             const long long* __restrict__ out_off, long long out_numel, int n_x,
                                                             int k, int b, int s, int w_l_c, int w_h_c, int elev_log, ElevRange e) {
  const int scene = blockIdx.y;
  const long long total = (long long)w_h_c * w_h_c;
  const long long off = out_off[scene];
  if (off < 0 || off + total > out_numel) return;               // a mosaic that leaves the pooled buffer is not written
  const float* __restrict__ t0 = tiles + (size_t)scene * n_x * n_x * k * k;
  float* __restrict__ o = out + off;
  const float bs = base[scene];
  const int p = w_l_c - s;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int X = (int)(i % w_h_c), Y = (int)(i / w_h_c);
    if (n_x == 1) {                                             // the 8 m case: the de-scaled tile, uncropped
      o[i] = to_metres(t0[i], elev_log, e.lo, e.span, e.log_span, bs);
      continue;
    }
    float acc = 0.f;
    for (int r = 0; r < n_x; ++r) {
      const int jy = Y - s * r;
      if (jy < 0 || jy >= w_l_c) continue;
      const float wy = ramp_weight(ramp, p, w_l_c, n_x, r, jy);
      for (int c = 0; c < n_x; ++c) {
        const int jx = X - s * c;
        if (jx < 0 || jx >= w_l_c) continue;
        const float wx = ramp_weight(ramp, p, w_l_c, n_x, c, jx);
        const float t = to_metres(t0[((size_t)(r * n_x + c) * k + b + jy) * k + b + jx], elev_log, e.lo, e.span, e.log_span, bs);
        acc = feather_add(acc, t, wx, wy);
      }
    }
    o[i] = acc;
  }
}

// ---- (b) pooled scores ---------------------------------------------------------------------------------------------
struct Mask {                // K18, by value in the kernel arguments; all null in the unmasked instances, never read there
  const unsigned char* plane;  // the validity plane, the ground truth's layout and numel
  unsigned char* keep;         // [total] a byte per pooled element, the layout of one candidate's e
  unsigned* chunk_n;           // [total_chunks] valid elements per chunk
  long long* counts;           // [n_seg] the output
};

// The chunk of a segment this workgroup owns: segment, its start in e, the element range [lo, hi) inside the segment.
__device__ __forceinline__ bool my_chunk(const long long* __restrict__ seg, int n_seg, long long total, int reps, int& s, long long& e_start,
                                         long long& lo, long long& hi, int& rep) {
  s = find_row(seg, n_seg, SEG_WORDS, 2, (long long)blockIdx.x);
  const long long* sg = seg + (size_t)s * SEG_WORDS;
  e_start = sg[0];
  const long long n = sg[1];
  const long long ch = (long long)blockIdx.x - sg[2];
  rep = (int)(ch & (reps - 1));                                  // reps is a power of two
  lo = ch * CHUNK;
  if (lo < 0 || lo >= n || e_start < 0 || e_start + n > total) return false;   // a table that leaves the workspace: nothing is touched
  hi = lo + CHUNK < n ? lo + CHUNK : n;
  return true;
}

template <bool MASKED>
__global__ __launch_bounds__(MT) void summary_prepare_kernel(Buffers B, Mask K, const long long* __restrict__ win, int n_win,
                                                            const long long* __restrict__ seg, int n_seg, long long total,
                                                            long long total_chunks, int reps, float* __restrict__ e_all,
                                                            double* __restrict__ partial, unsigned* __restrict__ hist) {
  __shared__ unsigned lh[2][256];
  __shared__ double red[MT / 64];
  __shared__ unsigned nred[MT / 64];
  const int tid = threadIdx.x, c = blockIdx.y;
  lh[0][tid] = 0u;
  lh[1][tid] = 0u;
  int s, rep;
  long long e_start, lo, hi;
  if (!my_chunk(seg, n_seg, total, reps, s, e_start, lo, hi, rep)) return;      // workgroup-uniform
  __syncthreads();
  float* __restrict__ e = e_all + (size_t)c * total;
  WindowCursor W(B, c);
  double sum = 0.0;
  unsigned kept = 0u;                                           // MASKED: valid elements this thread has seen
  for (long long base = lo; base < hi; base += MT * UNROLL) {
    float err[UNROLL];
    bool valid[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long long i = base + u * MT + tid;
      valid[u] = i < hi;
      err[u] = 0.f;
      if (!valid[u]) continue;
      const long long p = e_start + i;
      float v;                                                  // a NaN: an element no window of segment s covers, or a read outside a buffer
      bool keep = true;                                         // ... counts as valid: the row turns NaN, as without a mask
      pooled_fetch(W, win, n_win, p, v, [&](long long jg) {
        if constexpr (MASKED) keep = K.plane[jg] != 0;            // the plane has gt's numel (checked by the entry)
      }, s);
      if constexpr (MASKED) {
        if (!keep) v = 0.f;                                     // whatever cand and gt hold there: it is never looked at again
        if (c == 0) K.keep[p] = keep ? 1 : 0;
        valid[u] = keep;                                        // masked lanes still arrive at hist_add, with match = false
        kept += keep ? 1u : 0u;
      }
      err[u] = v;
      e[p] = v;
      if (keep) sum += (double)v * (double)v;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      hist_add(lh[0], valid[u], order_key(err[u]) >> 24);
      hist_add(lh[1], valid[u], order_key(fabsf(err[u])) >> 24);
    }
  }
  const double v = wave_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  if constexpr (MASKED) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) kept += (unsigned)__shfl_xor((int)kept, d, 64);
    if ((tid & 63) == 0) nred[tid >> 6] = kept;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int q = 0; q < MT / 64; ++q) t += red[q];
    partial[(size_t)c * total_chunks + blockIdx.x] = t;
    if constexpr (MASKED) {
      if (c == 0) {
        unsigned nk = 0u;
        for (int q = 0; q < MT / 64; ++q) nk += nred[q];
        K.chunk_n[blockIdx.x] = nk;
      }
    }
  }
  unsigned* hrow = hist + (((size_t)c * n_seg + s) * reps + rep) * NSTATE * 256;
  if (lh[0][tid]) atomicAdd(&hrow[0 * 256 + tid], lh[0][tid]);
  if (lh[1][tid]) atomicAdd(&hrow[2 * 256 + tid], lh[1][tid]);
}

// histograms of byte `pass` of the keys that carry their state's prefix.  group 0: states 0..3 (e and |e|, one read for
// both); group 1: states 4, 5 (|e - median|).  While the two states of a pair agree on the higher bytes, only the lower
// one is counted (the scan reads it for both).
template <bool MASKED>
__global__ __launch_bounds__(MT) void summary_select_kernel(const float* __restrict__ e_all, Mask K, const long long* __restrict__ seg, int n_seg,
                                                           long long total, int reps, int group, int pass, const RowState* __restrict__ st,
                                                           unsigned* __restrict__ hist) {
  __shared__ unsigned lh[4][256];
  const int tid = threadIdx.x, c = blockIdx.y;
#pragma unroll
  for (int q = 0; q < 4; ++q) lh[q][tid] = 0u;
  int s, rep;
  long long e_start, lo, hi;
  if (!my_chunk(seg, n_seg, total, reps, s, e_start, lo, hi, rep)) return;
  __syncthreads();
  const size_t row = (size_t)c * n_seg + s;
  const RowState* my = st + row;
  const int shift = pass * 8;
  const unsigned himask = pass == 3 ? 0u : (0xffffffffu << (shift + 8));
  const int q0 = group ? 4 : 0;
  const unsigned pa0 = my->prefix[q0] & himask, pa1 = my->prefix[q0 + 1] & himask;
  const unsigned pb0 = group ? 0u : my->prefix[2] & himask, pb1 = group ? 0u : my->prefix[3] & himask;
  const bool split_a = pa0 != pa1, split_b = pb0 != pb1;      // workgroup-uniform
  const float center = my->center;
  const float* __restrict__ e = e_all + (size_t)c * total + e_start;
  for (long long base = lo; base < hi; base += MT * UNROLL) {
    float x[UNROLL];
    bool valid[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const long long i = base + u * MT + tid;
      valid[u] = i < hi;
      x[u] = valid[u] ? e[i] : 0.f;
      if constexpr (MASKED) valid[u] = valid[u] && K.keep[e_start + i] != 0;     // e_start + i < total (my_chunk)
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const unsigned ka = order_key(group ? fabsf(__fsub_rn(x[u], center)) : x[u]);
      const unsigned bin_a = (ka >> shift) & 0xffu;
      hist_add(lh[0], valid[u] && (ka & himask) == pa0, bin_a);
      if (split_a) hist_add(lh[1], valid[u] && (ka & himask) == pa1, bin_a);
      if (!group) {
        const unsigned kb = order_key(fabsf(x[u]));
        const unsigned bin_b = (kb >> shift) & 0xffu;
        hist_add(lh[2], valid[u] && (kb & himask) == pb0, bin_b);
        if (split_b) hist_add(lh[3], valid[u] && (kb & himask) == pb1, bin_b);
      }
    }
  }
  __syncthreads();
  unsigned* hrow = hist + (row * reps + rep) * NSTATE * 256;
  const int nq = group ? 2 : 4;
  for (int q = 0; q < nq; ++q)
    if (lh[q][tid]) atomicAdd(&hrow[(q0 + q) * 256 + tid], lh[q][tid]);
}

// One workgroup per (candidate, segment): rank_scan (summary_select.h) behind this kernel's own init block.  init: the
// first scan of a call -- RMSE / PSNR from the chunk sums, folded in chunk order; the count, the ranks and the LE95 weight
// from the segment table, or (MASKED) the count from the chunk counts and the ranks formed here from it.
template <bool MASKED>
__global__ __launch_bounds__(MT) void summary_scan_kernel(const double* __restrict__ partial, Mask K, long long total_chunks,
                                                         const long long* __restrict__ seg, int n_seg, int reps, int group,
                                                         int pass, int init, double value_max, RowState* __restrict__ st,
                                                         unsigned* __restrict__ hist, float* __restrict__ out) {
  __shared__ RowState cur;
  __shared__ double red[MT / 64];
  __shared__ long long nred[MT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t row = blockIdx.x;
  const int c = (int)(row / n_seg), s = (int)(row % n_seg);
  const long long* sg = seg + (size_t)s * SEG_WORDS;
  const long long n = sg[1];
  unsigned* hrow = hist + row * reps * NSTATE * 256;           // the row's `reps` replicas, back to back
  float* o = out + row * NOUT;
  if (init) {
    if (tid == 0) {
      for (int q = 0; q < NSTATE; ++q) cur.prefix[q] = 0u;
      if constexpr (!MASKED) {
        cur.k[0] = cur.k[4] = (unsigned)sg[3];
        cur.k[1] = cur.k[5] = (unsigned)sg[4];
        cur.k[2] = (unsigned)sg[5];
        cur.k[3] = (unsigned)sg[6];
      }
      cur.center = 0.f;
      cur.has_nan = 0u;
      cur.g[0] = cur.g[1] = 0u;
    }
    const long long nchunks = (n + CHUNK - 1) / CHUNK;
    const double* src = partial + (size_t)c * total_chunks + sg[2];
    double a = 0.0;
    if (sg[2] >= 0 && sg[2] + nchunks <= total_chunks)
      for (long long j = tid; j < nchunks; j += MT) a += src[j];
    a = wave_sum(a);
    if (lane == 0) red[wave] = a;
    if constexpr (MASKED) {                                      // n_v: integers, exact in any order
      long long nk = 0;
      if (sg[2] >= 0 && sg[2] + nchunks <= total_chunks)
        for (long long j = tid; j < nchunks; j += MT) nk += (long long)K.chunk_n[sg[2] + j];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) nk += __shfl_xor(nk, d, 64);
      if (lane == 0) nred[wave] = nk;
    }
  } else if (tid < (int)(sizeof(RowState) / 4)) {
    reinterpret_cast<unsigned*>(&cur)[tid] = reinterpret_cast<const unsigned*>(st + row)[tid];
  }
  __syncthreads();
  if (init && tid == 0) {
    double t = 0.0;
    for (int q = 0; q < MT / 64; ++q) t += red[q];
    long long n_v = n;
    if constexpr (MASKED) {
      n_v = 0;
      for (int q = 0; q < MT / 64; ++q) n_v += nred[q];
      if (n_v < 0 || n_v > n) n_v = 0;                           // cannot happen with counts this call wrote
      if (c == 0) K.counts[s] = n_v;
      if (n_v >= 1) {
        const Ranks r = segment_ranks_of(n_v);
        cur.k[0] = cur.k[4] = (unsigned)r.m0;
        cur.k[1] = cur.k[5] = (unsigned)r.m1;
        cur.k[2] = (unsigned)r.l0;
        cur.k[3] = (unsigned)r.l1;
        __builtin_memcpy(cur.g, &r.g, 8);
      } else {                                                   // every histogram of the row stays empty: no lane finds a rank
        for (int q = 0; q < NSTATE; ++q) cur.k[q] = 0u;
      }
    }
    const double rm = sqrt(t / (double)n_v);
    o[0] = (float)rm;
    o[4] = (float)(20.0 * log10(value_max / rm));               // +inf at rm == 0; NaN stays NaN
    cur.has_nan = (t != t) ? 1u : 0u;
    if constexpr (MASKED) cur.has_nan |= n_v < 1 ? 2u : 0u;
  }
  if constexpr (MASKED) {
    if (init) __syncthreads();                                   // kernel-uniform: the ranks were written after the barrier above
  }
  rank_scan(cur, MASKED ? static_cast<const void*>(cur.g) : static_cast<const void*>(sg + 7), hrow, reps, group, pass, o, st + row);
}

bool sizes_ok(int n_cand, int n_segments, long long total, long long total_chunks) {
  if (n_cand < 1 || n_cand > MAXC || n_segments <= 0 || total <= 0 || total >= 0x100000000ll) return false;
  // every segment holds at least one element and ends in at most one partly filled chunk
  return n_segments <= total && total_chunks >= (total + CHUNK - 1) / CHUNK && total_chunks <= total / CHUNK + n_segments &&
         total_chunks < 0x7fffffffll;
}

}  // namespace

extern "C" int jspsr_scenes_assemble_f32(const float* tiles, const float* base, const float* ramp, float* out, const long long* out_off,
                                         long long out_numel, int S, int n_x, int k, int border_px, int stride, int elev_log,
                                         double elev_min, double elev_max, jspsr_stream_t stream) {
  if (!tiles || !base || !out || !out_off || out_numel <= 0 || S <= 0 || n_x <= 0 || k <= 0 || border_px < 0)
    return fail(JSPSR_EINVAL, "scenes_assemble: bad arguments");
  if (S > 65535) return fail(JSPSR_EINVAL, "scenes_assemble: S = %d exceeds the grid (65535)", S);
  if (!(elev_max > elev_min)) return fail(JSPSR_EINVAL, "scenes_assemble: elev_max must exceed elev_min");
  int w_l_c = k, w_h_c = k, b = 0, p = 0;
  if (n_x > 1) {
    b = border_px;
    w_l_c = k - 2 * b;
    w_h_c = stride * (n_x - 1) + w_l_c;
    p = w_l_c - stride;
    if (w_l_c <= 0 || stride <= 0 || p < 0 || (p > 0 && !ramp) || p > w_l_c) return fail(JSPSR_EINVAL, "scenes_assemble: bad cover");
  }
  const long long total = (long long)w_h_c * w_h_c;
  long long blocks = (total + 255) / 256;
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(scenes_assemble_kernel, dim3((unsigned)blocks, S), dim3(256), 0, static_cast<hipStream_t>(stream), tiles, base, ramp,
                     out, out_off, out_numel, n_x, k, b, stride, w_l_c, w_h_c, elev_log ? 1 : 0, elev_range(elev_min, elev_max));
  return check_launch("scenes_assemble");
}


namespace {

// The workspace: e, the chunk sums, the histograms, [K18: the chunk counts, cleared with the histograms], the row states,
// [K18: the validity bytes].  The unmasked layout is K12's.
size_t workspace_bytes(bool masked, int n_cand, int n_segments, long long total, long long total_chunks) {
  if (!sizes_ok(n_cand, n_segments, total, total_chunks)) return 0;
  const size_t rows = (size_t)n_cand * n_segments;
  const size_t k12 = up16((size_t)n_cand * total * sizeof(float)) + up16((size_t)n_cand * total_chunks * sizeof(double)) +
                     rows * hist_replicas(rows, total_chunks) * NSTATE * 256 * sizeof(unsigned) + rows * sizeof(RowState) + 64;
  return masked ? k12 + up16((size_t)total_chunks * sizeof(unsigned)) + up16((size_t)total) : k12;
}

template <bool MASKED>
int summary_run(const char* name, const float* const* cands, const long long* cand_numel, int n_cand, const float* gt, long long gt_numel,
                const unsigned char* valid, long long valid_numel, const long long* windows, int n_windows, const long long* segments,
                int n_segments, long long total, long long total_chunks, double value_max, float* out, long long* counts,
                void* workspace, jspsr_stream_t stream) {
  if (n_cand < 1 || n_cand > MAXC) return fail(JSPSR_EINVAL, "%s: n_cand = %d is outside 1..%d", name, n_cand, MAXC);
  if (!cands || !cand_numel || !gt || !windows || !segments || !out || !workspace) return fail(JSPSR_EINVAL, "%s: null pointer", name);
  if (MASKED && (!valid || !counts)) return fail(JSPSR_EINVAL, "%s: null validity plane or counts", name);
  if (n_windows <= 0 || n_segments <= 0 || total <= 0 || gt_numel <= 0) return fail(JSPSR_EINVAL, "%s: empty window or segment table", name);
  if (MASKED && valid_numel != gt_numel)
    return fail(JSPSR_EINVAL, "%s: the validity plane has %lld elements, the ground truth %lld", name, valid_numel, gt_numel);
  if (total >= 0x100000000ll) return fail(JSPSR_EINVAL, "%s: %lld pooled elements, the rank counters hold fewer than 2^32", name, total);
  if (n_windows < n_segments || !sizes_ok(n_cand, n_segments, total, total_chunks))
    return fail(JSPSR_EINVAL, "%s: %d windows, %d segments, %lld elements and %lld chunks do not fit together", name, n_windows,
                n_segments, total, total_chunks);
  if ((long long)n_cand * n_segments > 0x7fffffffll) return fail(JSPSR_EINVAL, "%s: too many rows", name);
  Buffers B;
  if (int err = pack_buffers(name, cands, cand_numel, n_cand, gt, gt_numel, B)) return err;
  if (!aligned4(gt) || !aligned4(out)) return fail(JSPSR_EALIGN, "%s: tensors not 4-byte aligned", name);
  if (MASKED && (reinterpret_cast<uintptr_t>(counts) & 7u)) return fail(JSPSR_EALIGN, "%s: counts not 8-byte aligned", name);
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "%s: workspace not 16-byte aligned", name);
  const size_t rows = (size_t)n_cand * n_segments;
  char* ws = static_cast<char*>(workspace);
  float* e = reinterpret_cast<float*>(ws);
  size_t off = up16((size_t)n_cand * total * sizeof(float));
  double* partial = reinterpret_cast<double*>(ws + off);
  off += up16((size_t)n_cand * total_chunks * sizeof(double));
  unsigned* hist = reinterpret_cast<unsigned*>(ws + off);
  const int reps = hist_replicas(rows, total_chunks);
  const size_t hist_bytes = rows * reps * NSTATE * 256 * sizeof(unsigned);
  off += hist_bytes;
  size_t clear_bytes = hist_bytes;
  Mask K = {nullptr, nullptr, nullptr, nullptr};
  if (MASKED) {
    K.plane = valid;
    K.counts = counts;
    K.chunk_n = reinterpret_cast<unsigned*>(ws + off);            // behind the histograms: one clear serves both
    off += up16((size_t)total_chunks * sizeof(unsigned));
    clear_bytes = off - (size_t)(reinterpret_cast<char*>(hist) - ws);
  }
  RowState* st = reinterpret_cast<RowState*>(ws + off);
  if (MASKED) K.keep = reinterpret_cast<unsigned char*>(ws + off + rows * sizeof(RowState) + 64);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(hist, 0, clear_bytes, s) != hipSuccess)
    return fail(JSPSR_EINVAL, "%s: clearing the histograms failed: %s", name, hipGetErrorString(hipGetLastError()));
  // the census labels (string literals, found by pointer): the scans count as selects, as in K12
  const char* const prepare_label = MASKED ? "summary_valid_prepare" : "summary_prepare";
  const char* const select_label = MASKED ? "summary_valid_select" : "summary_select";
  const dim3 grid((unsigned)total_chunks, n_cand);
  hipLaunchKernelGGL(summary_prepare_kernel<MASKED>, grid, dim3(MT), 0, s, B, K, windows, n_windows, segments, n_segments, total,
                     total_chunks, reps, e, partial, hist);
  if (int err = check_launch(prepare_label)) return err;
  for (int group = 0; group < 2; ++group) {
    for (int pass = 3; pass >= 0; --pass) {
      const int init = group == 0 && pass == 3;                  // the top digit of e and |e| was counted by the first pass
      if (!init) {
        hipLaunchKernelGGL(summary_select_kernel<MASKED>, grid, dim3(MT), 0, s, e, K, segments, n_segments, total, reps, group, pass, st,
                           hist);
        if (int err = check_launch(select_label)) return err;
      }
      hipLaunchKernelGGL(summary_scan_kernel<MASKED>, dim3((unsigned)rows), dim3(MT), 0, s, partial, K, total_chunks, segments, n_segments,
                         reps, group, pass, init, value_max, st, hist, out);
      if (int err = check_launch(select_label)) return err;
    }
  }
  return JSPSR_OK;
}

}  // namespace

extern "C" size_t jspsr_summary_workspace_bytes(int n_cand, int n_segments, long long total, long long total_chunks) {
  return workspace_bytes(false, n_cand, n_segments, total, total_chunks);
}

extern "C" int jspsr_summary_forward(const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                                     long long gt_numel, const long long* windows, int n_windows, const long long* segments,
                                     int n_segments, long long total, long long total_chunks, double value_max, float* out,
                                     void* workspace, jspsr_stream_t stream) {
  return summary_run<false>("summary_forward", cands, cand_numel, n_cand, gt, gt_numel, nullptr, 0, windows, n_windows, segments, n_segments,
                            total, total_chunks, value_max, out, nullptr, workspace, stream);
}

extern "C" size_t jspsr_summary_valid_workspace_bytes(int n_cand, int n_segments, long long total, long long total_chunks) {
  return workspace_bytes(true, n_cand, n_segments, total, total_chunks);
}

extern "C" int jspsr_summary_valid_forward(const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                                           long long gt_numel, const unsigned char* valid, long long valid_numel,
                                           const long long* windows, int n_windows, const long long* segments, int n_segments,
                                           long long total, long long total_chunks, double value_max, float* out, long long* counts,
                                           void* workspace, jspsr_stream_t stream) {
  return summary_run<true>("summary_valid_forward", cands, cand_numel, n_cand, gt, gt_numel, valid, valid_numel, windows, n_windows,
                           segments, n_segments, total, total_chunks, value_max, out, counts, workspace, stream);
}

extern "C" int jspsr_summary_ranks(long long n, long long* out5) {
  if (n < 1 || !out5) return fail(JSPSR_EINVAL, "summary_ranks: n = %lld (n >= 1 and a non-null result are taken)", n);
  const Ranks r = segment_ranks_of(n);
  out5[0] = r.m0;
  out5[1] = r.m1;
  out5[2] = r.l0;
  out5[3] = r.l1;
  __builtin_memcpy(&out5[4], &r.g, 8);
  return JSPSR_OK;
}
