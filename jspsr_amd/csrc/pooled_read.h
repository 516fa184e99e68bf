// How the pooled kernels read their input: csrc/summary.hip (K12, K18), csrc/errdist.hip (K21) and csrc/strata.hip (K22)
// walk one pool of e = cand - gt through the same table of pitched windows.  The candidates' buffers by value in the
// kernel arguments, the entry points' check and packing of them, the window a thread read last and the fetch of one
// pooled element.
#pragma once
#include "common.h"
#include "summary_select.h"

namespace jspsr {

constexpr int MAXC = 8;                       // candidates of a call
constexpr int WIN_WORDS = 4 + 2 * (1 + MAXC); // a window row: segment, h, w, e offset, {offset, pitch} of gt, cand 0..7

struct Buffers {             // by value in the kernel arguments
  const float* cand[MAXC];
  long long cand_numel[MAXC];
  const float* gt;
  long long gt_numel;
};

// The candidates of an entry point -> B, refused under the entry's own name: a null or empty one, then a misaligned one,
// candidate by candidate.  Every other check stays with the entry, in its own order.
inline int pack_buffers(const char* name, const float* const* cands, const long long* cand_numel, int n_cand, const float* gt,
                        long long gt_numel, Buffers& B) {
  for (int c = 0; c < MAXC; ++c) {
    B.cand[c] = c < n_cand ? cands[c] : nullptr;
    B.cand_numel[c] = c < n_cand ? cand_numel[c] : 0;
    if (c < n_cand && (!cands[c] || cand_numel[c] <= 0)) return fail(JSPSR_EINVAL, "%s: candidate %d is null or empty", name, c);
    if (c < n_cand && !aligned4(cands[c])) return fail(JSPSR_EALIGN, "%s: candidate %d not 4-byte aligned", name, c);
  }
  B.gt = gt;
  B.gt_numel = gt_numel;
  return JSPSR_OK;
}

struct WindowCursor {        // a thread's view of candidate c: its buffers and the window of the last element it read
  const float* __restrict__ cp;
  const float* __restrict__ gp;
  long long cn, gn;
  int c;
  long long lo = 0, hi = 0, w = 1, goff = 0, gpitch = 0, coff = 0, cpitch = 0;
  bool ok = false;
  __device__ __forceinline__ WindowCursor(const Buffers& B, int cand) : cp(B.cand[cand]), gp(B.gt), cn(B.cand_numel[cand]), gn(B.gt_numel), c(cand) {}
};

// Pooled element p of the cursor's candidate: e = cand - gt, and at_gt(jg) with the ground truth's index, where the caller
// reads its own planes in gt's layout.  at_gt runs beside the two reads of the subtraction, in one block: the loads of a
// caller's plane are issued with them, not behind them.  The window is found by bisection on the table's e offsets when p
// leaves the cursor's; segment >= 0: a window of another segment does not count.  false, with e a NaN and at_gt not
// called: no window covers p, or a read outside a buffer.
template <class AtGt>
__device__ __forceinline__ bool pooled_fetch(WindowCursor& W, const long long* __restrict__ win, int n_win, long long p, float& e,
                                             AtGt&& at_gt, int segment = -1) {
  const int c = W.c;
  if (p < W.lo || p >= W.hi) {
    const long long* wr = win + (size_t)find_row(win, n_win, WIN_WORDS, 3, p) * WIN_WORDS;
    W.w = wr[2];
    W.lo = wr[3];
    W.hi = W.lo + wr[1] * W.w;
    W.ok = ((segment < 0) | (wr[0] == segment)) && wr[1] > 0 && W.w > 0;     // | : no branch for the optional test
    W.goff = wr[4]; W.gpitch = wr[5];
    W.coff = wr[6 + 2 * c]; W.cpitch = wr[7 + 2 * c];
  }
  if (W.ok && p >= W.lo && p < W.hi) {
    const long long local = p - W.lo;
    long long y;
    if (local < 0x100000000ll && W.w < 0x100000000ll) y = (long long)((unsigned)local / (unsigned)W.w);   // the usual case: a 32-bit division
    else y = local / W.w;
    const long long x = local - y * W.w;
    const long long jc = W.coff + y * W.cpitch + x, jg = W.goff + y * W.gpitch + x;
    if (jc >= 0 && jc < W.cn && jg >= 0 && jg < W.gn) {
      e = __fsub_rn(W.cp[jc], W.gp[jg]);
      at_gt(jg);
      return true;
    }
  }
  e = __builtin_nanf("");
  return false;
}

}  // namespace jspsr
