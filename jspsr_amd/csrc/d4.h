// The D4 index maps of K14 and K16 (scene_prepare.hip, scene_tta.hip): code = rot90 * 4 + flip_lr * 2 + flip_ud, the
// transformed raster flipud?(fliplr?(rot90(m, rot90))), W x H for an odd rot90.  Integers only: the same map in every
// translation unit that includes this.
#pragma once
#include "common.h"

namespace jspsr {

// Pixel (i, j) of flipud?(fliplr?(rot90(m, angle))) is pixel (sy, sx) of the H x W raster m: K9's d4_source (csrc/batch.hip)
// for a rectangle.  The transformed raster is W x H for an odd angle.
__device__ __forceinline__ void d4_source(int code, int H, int W, int i, int j, int& sy, int& sx) {
  const int odd = (code >> 2) & 1;
  const int i2 = (code & 1) ? (odd ? W : H) - 1 - i : i;
  const int j2 = (code & 2) ? (odd ? H : W) - 1 - j : j;
  switch (code >> 2) {
    case 0: sy = i2; sx = j2; break;
    case 1: sy = j2; sx = W - 1 - i2; break;          // np.rot90(m, 1)[i][j] = m[j][W-1-i]
    case 2: sy = H - 1 - i2; sx = W - 1 - j2; break;
    default: sy = H - 1 - j2; sx = i2; break;          // np.rot90(m, 3)[i][j] = m[H-1-j][i]
  }
}

// The other direction: pixel (y, x) of m is pixel (i, j) of the transformed raster
__device__ __forceinline__ void d4_image(int code, int H, int W, int y, int x, int& i, int& j) {
  const int odd = (code >> 2) & 1;
  int i2, j2;
  switch (code >> 2) {
    case 0: i2 = y; j2 = x; break;
    case 1: i2 = W - 1 - x; j2 = y; break;
    case 2: i2 = H - 1 - y; j2 = W - 1 - x; break;
    default: i2 = x; j2 = H - 1 - y; break;
  }
  i = (code & 1) ? (odd ? W : H) - 1 - i2 : i2;
  j = (code & 2) ? (odd ? H : W) - 1 - j2 : j2;
}

}  // namespace jspsr
