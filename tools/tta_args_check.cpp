// The argument checks of the two K14 entry points (csrc/scene_prepare.hip, scene_tta.hip) from a stand-alone program: null and invalid
// arguments, every call must come back with its code and message before a launch.  It needs no GPU and is meant for a host
// sanitizer build, from jspsr_amd/csrc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         scene_prepare.hip scene_tta.hip common.hip ../../tools/tta_args_check.cpp -o /tmp/tta_args_check && /tmp/tta_args_check
#include <cstdio>
#include <cstring>
#include "../include/jspsr_hip.h"
static int fails = 0;
#define EXPECT(call, code, text) do { int r = (call); const char* m = jspsr_last_error(); \
  if (r != (code) || !strstr(m, text)) { printf("FAIL %s -> %d '%s'\n", #call, r, m); ++fails; } } while (0)
int main() {
  void* x = (void*)4096;
  jspsr_tta_variant even{x, 0, 0, 24, 16, 3, 3, 13, 10}, odd{x, 0, 4, 16, 24, 3, 3, 10, 13};
  jspsr_tta_variant v[9];
  for (auto& e : v) e = even;
  EXPECT(jspsr_scene_finish_mean(nullptr, 1, (float*)x, (int*)x, 1, 13, 10, 1, 1, -80, 933, nullptr), -1, "bad arguments");
  EXPECT(jspsr_scene_finish_mean(v, 0, (float*)x, (int*)x, 1, 13, 10, 1, 1, -80, 933, nullptr), -1, "0 variants");
  EXPECT(jspsr_scene_finish_mean(v, 9, (float*)x, (int*)x, 1, 13, 10, 1, 1, -80, 933, nullptr), -1, "9 variants");
  EXPECT(jspsr_scene_finish_mean(v, 2, (float*)x, (int*)x, 1, 13, 10, 1, 1, -80, 933, nullptr), -1, "same element");
  v[1] = odd; v[1].code = 11; v[1].Hp = 24; v[1].Wp = 16; v[1].h = 13; v[1].w = 10;
  EXPECT(jspsr_scene_finish_mean(v, 2, (float*)x, (int*)x, 1, 13, 10, 1, 1, -80, 933, nullptr), -1, "same element");
  v[0].top = 12;
  EXPECT(jspsr_scene_finish_mean(v, 1, (float*)x, (int*)x, 1, 13, 10, 1, 1, -80, 933, nullptr), -1, "leaves");
  v[0] = even; v[0].code = 4;
  EXPECT(jspsr_scene_finish_mean(v, 1, (float*)x, (int*)x, 1, 13, 10, 1, 1, -80, 933, nullptr), -1, "transforms to 10 x 13");
  v[0] = even; v[0].pred = (void*)4098;
  EXPECT(jspsr_scene_finish_mean(v, 1, (float*)x, (int*)x, 1, 13, 10, 1, 1, -80, 933, nullptr), -2, "aligned");
  v[0] = even;
  EXPECT(jspsr_scene_finish_mean(v, 1, (float*)x, (int*)x, 70000, 13, 10, 1, 1, -80, 933, nullptr), -1, "bad arguments");
  EXPECT(jspsr_scene_finish_mean(v, 1, (float*)x, (int*)x, 1, 13, 10, 1, 1, 5, 5, nullptr), -1, "bad arguments");

  const void* src[6] = {}; long long nbytes[6] = {}; float* out[6] = {}; int ch[6] = {}, coff[6] = {}, pitch[6] = {};
  int codes[3] = {0, 2, 8};
  out[5] = (float*)x; ch[5] = 2; pitch[5] = 2;
  EXPECT(jspsr_scene_prepare_d4(nullptr, nbytes, out, ch, coff, pitch, (long long*)x, 1, (int*)x, codes, 3, (int*)x, (int*)x, 24, 16, 0, -80, 933, 3, nullptr), -1, "bad arguments");
  EXPECT(jspsr_scene_prepare_d4(src, nbytes, out, ch, coff, pitch, (long long*)x, 1, (int*)x, nullptr, 3, (int*)x, (int*)x, 24, 16, 0, -80, 933, 3, nullptr), -1, "bad arguments");
  EXPECT(jspsr_scene_prepare_d4(src, nbytes, out, ch, coff, pitch, (long long*)x, 1, (int*)x, codes, 0, (int*)x, (int*)x, 24, 16, 0, -80, 933, 3, nullptr), -1, "bad arguments");
  codes[1] = 4;
  EXPECT(jspsr_scene_prepare_d4(src, nbytes, out, ch, coff, pitch, (long long*)x, 1, (int*)x, codes, 3, (int*)x, (int*)x, 24, 16, 0, -80, 933, 3, nullptr), -1, "one parity");
  codes[1] = 16;
  EXPECT(jspsr_scene_prepare_d4(src, nbytes, out, ch, coff, pitch, (long long*)x, 1, (int*)x, codes, 3, (int*)x, (int*)x, 24, 16, 0, -80, 933, 3, nullptr), -1, "outside 0..15");
  codes[1] = 2; out[5] = nullptr;
  EXPECT(jspsr_scene_prepare_d4(src, nbytes, out, ch, coff, pitch, (long long*)x, 1, (int*)x, codes, 3, (int*)x, (int*)x, 24, 16, 0, -80, 933, 3, nullptr), -1, "no output");
  out[3] = (float*)x; ch[3] = 2; pitch[3] = 2;
  EXPECT(jspsr_scene_prepare_d4(src, nbytes, out, ch, coff, pitch, (long long*)x, 1, (int*)x, codes, 3, (int*)x, (int*)x, 24, 16, 0, -80, 933, 3, nullptr), -1, "store");
  out[3] = (float*)4098;
  EXPECT(jspsr_scene_prepare_d4(src, nbytes, out, ch, coff, pitch, (long long*)x, 1, (int*)x, codes, 3, (int*)x, (int*)x, 24, 16, 0, -80, 933, 3, nullptr), -2, "aligned");
  printf("%s (%d failures)\n", fails ? "FAILED" : "all refused before a launch", fails);
  return fails != 0;
}
