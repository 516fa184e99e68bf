// The candidate check the three pooled entry points share (csrc/pooled_read.h: pack_buffers) from a stand-alone program:
// every call must come back with its code and its message, under the entry's own name, before a launch.  It needs no GPU
// and is meant for a host sanitizer build, from jspsr_amd/csrc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         summary.hip strata.hip errdist.hip common.hip ../../tools/pooled_args_check.cpp -o /tmp/pooled_args_check && /tmp/pooled_args_check
#include <cstdio>
#include <cstring>
#include "../include/jspsr_hip.h"
static int fails = 0;
#define EXPECT(call, code, text) do { int r = (call); const char* m = jspsr_last_error(); \
  if (r != (code) || !strstr(m, text)) { printf("FAIL %s -> %d '%s'\n", #call, r, m); ++fails; } } while (0)
int main() {
  float* x = (float*)4096;
  unsigned char* u = (unsigned char*)4096;
  long long* q = (long long*)4096;
  const float* good[8] = {x, x, x, x, x, x, x, x};
  const float* null2[3] = {x, x, nullptr};
  const float* odd1[2] = {x, (const float*)4098};
  const long long numel[8] = {64, 64, 64, 64, 64, 64, 64, 64}, empty1[2] = {64, 0};
  // K12 / K18: one segment of 64 elements in one window and one chunk
  EXPECT(jspsr_summary_forward(null2, numel, 3, x, 64, q, 1, q, 1, 64, 1, 933.0, x, x, nullptr), -1, "summary_forward: candidate 2 is null or empty");
  EXPECT(jspsr_summary_forward(good, empty1, 2, x, 64, q, 1, q, 1, 64, 1, 933.0, x, x, nullptr), -1, "summary_forward: candidate 1 is null or empty");
  EXPECT(jspsr_summary_forward(odd1, numel, 2, x, 64, q, 1, q, 1, 64, 1, 933.0, x, x, nullptr), -2, "summary_forward: candidate 1 not 4-byte aligned");
  EXPECT(jspsr_summary_forward(good, numel, 9, x, 64, q, 1, q, 1, 64, 1, 933.0, x, x, nullptr), -1, "n_cand = 9");
  EXPECT(jspsr_summary_forward(good, numel, 8, (const float*)4098, 64, q, 1, q, 1, 64, 1, 933.0, x, x, nullptr), -2, "tensors not 4-byte aligned");
  EXPECT(jspsr_summary_valid_forward(null2, numel, 3, x, 64, u, 64, q, 1, q, 1, 64, 1, 933.0, x, q, x, nullptr), -1,
         "summary_valid_forward: candidate 2 is null or empty");
  EXPECT(jspsr_summary_valid_forward(odd1, numel, 2, x, 64, u, 64, q, 1, q, 1, 64, 1, 933.0, x, q, x, nullptr), -2,
         "summary_valid_forward: candidate 1 not 4-byte aligned");
  EXPECT(jspsr_summary_valid_forward(odd1, numel, 2, x, 64, u, 63, q, 1, q, 1, 64, 1, 933.0, x, q, x, nullptr), -1, "validity plane has 63");
  // K22
  EXPECT(jspsr_strata_forward(null2, numel, 3, x, 64, u, 64, 4, nullptr, 0, q, 1, 64, 933.0, x, q, x, nullptr), -1,
         "strata_forward: candidate 2 is null or empty");
  EXPECT(jspsr_strata_forward(odd1, numel, 2, x, 64, u, 64, 4, nullptr, 0, q, 1, 64, 933.0, x, q, x, nullptr), -2,
         "strata_forward: candidate 1 not 4-byte aligned");
  EXPECT(jspsr_strata_forward(odd1, numel, 2, x, 64, u, 63, 4, nullptr, 0, q, 1, 64, 933.0, x, q, x, nullptr), -1, "label plane has 63");
  EXPECT(jspsr_strata_forward(good, numel, 8, x, 64, u, 64, 4, nullptr, 0, q, 1, 64, 933.0, x, (long long*)4100, x, nullptr), -2, "counts not 8-byte aligned");
  // K21
  EXPECT(jspsr_errdist_hist_forward(null2, numel, 3, x, 64, nullptr, 0, q, 1, 64, -5.0, 5.0, q, q, nullptr), -1,
         "errdist_hist_forward: candidate 2 is null or empty");
  EXPECT(jspsr_errdist_hist_forward(good, empty1, 2, x, 64, nullptr, 0, q, 1, 64, -5.0, 5.0, q, q, nullptr), -1,
         "errdist_hist_forward: candidate 1 is null or empty");
  EXPECT(jspsr_errdist_hist_forward(odd1, numel, 2, x, 64, nullptr, 0, q, 1, 64, -5.0, 5.0, q, q, nullptr), -2,
         "errdist_hist_forward: candidate 1 not 4-byte aligned");
  EXPECT(jspsr_errdist_hist_forward(odd1, numel, 2, x, 64, nullptr, 0, q, 1, 64, 5.0, -5.0, q, q, nullptr), -1, "lo = 5, hi = -5");
  EXPECT(jspsr_errdist_hist_forward(good, numel, 8, (const float*)4098, 64, nullptr, 0, q, 1, 64, -5.0, 5.0, q, q, nullptr), -2,
         "ground truth not 4-byte aligned");
  printf("%s (%d failures)\n", fails ? "FAILED" : "all refused before a launch", fails);
  return fails != 0;
}
