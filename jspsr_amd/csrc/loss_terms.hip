// The rest of the reference's loss menu (losses/loss_schemes.py:6-33, utils/common_config.py:209-233) on fp32
// (planes, H, W) tensors, beside the fused L1 + L2 + Sobel pair of train_step.hip:
//   * pointwise terms, one pass: BerHu (loss_functions.py:191-208), BCE-with-logits (nn.BCEWithLogitsLoss) and the
//     surface-normal loss of a one-channel map (:211-229).  BerHu's threshold 0.6 max|pred - gt| comes from a max pass
//     before the sum pass and stays in the workspace (no host round trip; a captured graph replays it).
//   * SSIM (SSIMLoss :232-239 = 1 - piq.ssim(clamp(pred,0,1), gt, data_range=1, downsample=False)): five 11x11 window
//     moments per map element, separable (an 11-tap horizontal then an 11-tap vertical pass out of LDS), valid mode for
//     the loss; zero-padded "same" mode with a caller's window for the local meter (evaluation/metrics.py:20-63).  The
//     forward writes the three per-element coefficients of dS/d(moment) so that the backward is the adjoint filter of
//     those three maps plus an epilogue.
// Every reduction writes per-workgroup partials folded in a fixed order in double: the same bits on every run.
// Gradients accumulate (+=) into a buffer the caller has already written.
#include "common.h"
#include "loss_fold.h"

#include <cmath>
#include <type_traits>

namespace {

using namespace jspsr;

constexpr int PT = 256;          // pointwise workgroup
constexpr int ST = 32;           // SSIM tile edge (map elements forward, pixels backward)
constexpr int SH = ST + 10;      // staged edge: tile + 10-px halo of the 11-tap window
constexpr int SN = 256;          // SSIM workgroup: 8 row groups x 32 columns, 4 rows each
constexpr float C1 = 1e-4f;      // (0.01 * data_range)^2
constexpr float C2 = 9e-4f;      // (0.03 * data_range)^2

enum { T_BERHU = 1, T_BCE = 2, T_NORM = 4, T_SSIM = 8, T_ALL = 15 };
enum { S_L1, S_L2, S_GRAD, S_BERHU, S_BCE, S_NORM, S_SSIM, NSLOT };
constexpr int MAXKEY = 16;

struct Win11 {
  float w[11];
};

struct KeyMap {             // the configured keys in config order: slot and weight of each
  int n;
  int slot[MAXKEY];
  double w[MAXKEY];
};

int pw_blocks(long long n) {
  long long b = (n + PT - 1) / PT;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// the max pass: few partials, since every workgroup of the sum pass folds all of them
int max_blocks(long long n) {
  long long b = (n + PT - 1) / PT;
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }

// piq's window: 11 taps, sigma 1.5, centred, normalised (the 2-D window is the outer product)
Win11 gaussian_window() {
  double g[11], s = 0.0;
  for (int i = 0; i < 11; ++i) { const double c = i - 5.0; g[i] = exp(-(c * c) / (2.0 * 1.5 * 1.5)); s += g[i]; }
  Win11 k;
  for (int i = 0; i < 11; ++i) k.w[i] = (float)(g[i] / s);
  return k;
}

// One workspace for the whole menu forward + backward, th[4] = {thf, th^2 as float, 2 th as float, -} at 0.  Unmasked: the
// pointwise partials only with a pointwise term.  Masked (K19, K23): always, then the per-workgroup counts and N (a long
// long in 16 bytes); SSIM's partials are followed by its counts and N_s in the same way.
struct Layout {
  int nb = 0, nbm = 0, nbs = 0, tiles_x = 0, tiles_y = 0, Hm = 0, Wm = 0;
  size_t pmax = 0, psum = 0, pcnt = 0, nn = 0, ssum = 0, scnt = 0, ns = 0, coef = 0, bytes = 0;
  long long cplane = 0;     // elements of one coefficient map set: planes * Hm * Wm
};

Layout layout(int terms, int planes, int H, int W, bool masked) {
  Layout L;
  const long long n = (long long)planes * H * W;
  L.nb = pw_blocks(n);
  L.nbm = max_blocks(n);
  size_t off = 16;
  if (masked || (terms & (T_BERHU | T_BCE | T_NORM))) {
    L.pmax = off; off += al16((size_t)L.nbm * 4);
    L.psum = off; off += al16((size_t)L.nb * 3 * 4);
  }
  if (masked) {
    L.pcnt = off; off += al16((size_t)L.nb * 4);
    L.nn = off; off += 16;
  }
  if (terms & T_SSIM) {
    L.Hm = H - 10; L.Wm = W - 10;
    L.tiles_x = (L.Wm + ST - 1) / ST; L.tiles_y = (L.Hm + ST - 1) / ST;
    L.nbs = L.tiles_x * L.tiles_y * planes;
    L.ssum = off; off += al16((size_t)L.nbs * 4);
    if (masked) {
      L.scnt = off; off += al16((size_t)L.nbs * 4);
      L.ns = off; off += 16;
    }
    L.cplane = (long long)planes * L.Hm * L.Wm;
    L.coef = off; off += al16((size_t)L.cplane * 3 * 4);
  }
  L.bytes = off;
  return L;
}

__device__ __forceinline__ float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// Block reduction of one float (sum or max) over SN/PT = 256 threads into lane 0 of wave 0 (fixed order).
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const float o = __shfl_xor(v, d, 64);
    v = MAX ? fmaxf(v, o) : v + o;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = MAX ? fmaxf(t, red[w]) : t + red[w];
  return t;
}

// ---- pointwise terms --------------------------------------------------------------------------------------------
// Per-element BerHu as torch evaluates the reference's expression with th a Python float: the comparison and both
// constants in fp32, no contraction of diff^2 + th^2.
__device__ __forceinline__ float berhu_elem(float ad, float thf, float t2f, float tw) {
#pragma clang fp contract(off)
  return ad <= thf ? ad : (ad * ad + t2f) / tw;
}

__device__ __forceinline__ float bce_elem(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))); }

__device__ __forceinline__ float unit(float v) { return v / fmaxf(fabsf(v), 1e-12f); }   // F.normalize, C = 1

// MASKED (K19): the terms over the elements a validity plane keeps.  valid: one byte per element, nonzero = valid.  pred / gt
// are used behind a select on the plane (never multiplied by it: NaN * 0 is NaN), in the same grids, loop order and fold
// order, one body per pass: an all-ones plane gives the unmasked bits.  N, the number of valid elements, is counted as an
// integer by the sum pass, folded by the combine kernel and left in the workspace for the backward.  N = 0: every term and
// every gradient element is 0.
template <bool MASKED>
__global__ __launch_bounds__(PT) void menu_max_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const unsigned char* __restrict__ valid, long long n,
                                                     float* __restrict__ pmax) {
  __shared__ float red[PT / 64];
  float m = 0.f;
  for (long long i = blockIdx.x * (long long)PT + threadIdx.x; i < n; i += (long long)gridDim.x * PT) {
    const float ad = fabsf(pred[i] - gt[i]);          // MASKED: loaded beside the plane's byte, not after it
    m = fmaxf(m, !MASKED || valid[i] ? ad : 0.f);
  }
  m = block_reduce<true>(m, red);
  if (threadIdx.x == 0) pmax[blockIdx.x] = m;
}

// partial sums {BerHu, BCE, 1 - p^.g^} per workgroup (MASKED: and the count of valid elements); block 0 stores BerHu's
// threshold for the backward
template <bool MASKED>
__global__ __launch_bounds__(PT) void menu_sum_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const unsigned char* __restrict__ valid, long long n, int terms,
                                                     const float* __restrict__ pmax, int nb, float* __restrict__ th,
                                                     float* __restrict__ psum, unsigned int* __restrict__ pcnt) {
  __shared__ float red[3 * (PT / 64)];
  __shared__ unsigned int redc[PT / 64];
  float thf = 0.f, t2f = 0.f, tw = 0.f;
  if (terms & T_BERHU) {
    float m = 0.f;
    for (int r = threadIdx.x; r < nb; r += PT) m = fmaxf(m, pmax[r]);
    m = block_reduce<true>(m, red);
    __syncthreads();
    const double t = 0.6 * (double)m;       // delta * torch.max(diff).item()
    thf = (float)t; t2f = (float)(t * t); tw = (float)(2.0 * t);
    if (blockIdx.x == 0 && threadIdx.x == 0) { th[0] = thf; th[1] = t2f; th[2] = tw; th[3] = 0.f; }
  }
  float s[3] = {0.f, 0.f, 0.f};
  unsigned int nv[1] = {0};
  for (long long i = blockIdx.x * (long long)PT + threadIdx.x; i < n; i += (long long)gridDim.x * PT) {
    const float x = pred[i], y = gt[i];               // MASKED: loaded beside the plane's byte, not after it
    if constexpr (MASKED) {
      if (!valid[i]) continue;
      ++nv[0];
    }
    if (terms & T_BERHU) s[0] += berhu_elem(fabsf(x - y), thf, t2f, tw);
    if (terms & T_BCE) s[1] += bce_elem(x, y);
    if (terms & T_NORM) s[2] += 1.f - unit(x) * unit(y);
  }
  block_fold3<PT, MASKED ? 1 : 0>(s, nv, red, redc, psum, pcnt);
}

// grad += up * (cb BerHu' + cc BCE' + cn Norm').  Unmasked: kb, kc, kn are the coefficients wb/n, wc/n, wn/(1e-12 n), formed
// by the host.  MASKED: they are the weights, and the coefficients (float)(w / (double)N) are formed here from the stored
// count (nothing valid: return, the caller's zeros stand); the gradient of an invalid element stays the +0.0 the caller wrote.
// BerHu's threshold is a constant (the reference detaches it by .item()); at th = 0 every element takes the |d| branch,
// whose gradient there is 0 (the reference: NaN, see header).
template <bool MASKED>
__global__ __launch_bounds__(PT) void menu_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const unsigned char* __restrict__ valid, long long n, int terms,
                                                     const float* __restrict__ th, const long long* __restrict__ nn,
                                                     const float* __restrict__ gscale,
                                                     std::conditional_t<MASKED, double, float> kb,
                                                     std::conditional_t<MASKED, double, float> kc,
                                                     std::conditional_t<MASKED, double, float> kn,
                                                     float* __restrict__ grad) {
  float cb, cc, cn;
  if constexpr (MASKED) {
    const long long nv = nn[0];
    if (nv <= 0) return;
    const double dn = (double)nv;
    cb = (float)(kb / dn); cc = (float)(kc / dn); cn = (float)(kn / (1e-12 * dn));
  } else {
    cb = kb; cc = kc; cn = kn;
  }
  const float up = gscale ? gscale[0] : 1.f;
  const float thf = (terms & T_BERHU) ? th[0] : 0.f, tw = (terms & T_BERHU) ? th[2] : 1.f;
  for (long long i = blockIdx.x * (long long)PT + threadIdx.x; i < n; i += (long long)gridDim.x * PT) {
    if constexpr (MASKED) {
      if (!valid[i]) continue;
    }
    const float x = pred[i], y = gt[i];
    float g = 0.f;
    if (terms & T_BERHU) {
      const float d = x - y, ad = fabsf(d);
      g += cb * (ad <= thf ? sgnf(d) : 2.f * ad / tw * sgnf(d));
    }
    if (terms & T_BCE) g += cc * (1.f / (1.f + expf(-x)) - y);
    if (terms & T_NORM) g += fabsf(x) <= 1e-12f ? -cn * unit(y) : 0.f;
    grad[i] += up * g;
  }
}

// ---- SSIM -------------------------------------------------------------------------------------------------------
// Forward over one ST x ST tile of the map of one plane.  SAME = false: valid map (H-10) x (W-10), map element q reads
// pixels q .. q+10; SAME = true: H x W map over the zero-padded plane, q reads q-5 .. q+5.  x = clamp(pred, 0, 1).
// coef (valid mode, may be NULL): alpha, beta, gamma of every map element, three planar maps cplane apart.
// MASKED (K23, the "window" rule): the planes are H x W windows of rasters with row stride ld and plane stride ps (the
// per-tile meter crops by index arithmetic), valid one byte per pixel beside them (NULL = every pixel valid).  The staged
// patch carries one BIT per pixel, 1 = an in-plane void (a wave's ballot is 64 consecutive pixels of the patch, so the
// flags cost no LDS traffic to speak of); pred and gt are staged as 0 there, behind a select.  Positions outside the
// plane are the zero padding, not voids.  "A void under the window" is formed separably, in integers, in the two passes
// of the moments: 11 bits of a row, then 11 rows of a column; a map element counts iff there is none.  S joins the
// partial, and alpha, beta, gamma are written, for counted elements only (zeros elsewhere: the backward's adjoint filter
// reads them); pcnt gets the workgroup's count.  Every float operation of a counted element is the unmasked kernel's.
template <bool SAME, bool MASKED>
__global__ __launch_bounds__(SN) void ssim_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     int H, int W, int Hm, int Wm, int tiles_x, Win11 k,
                                                     float* __restrict__ coef, long long cplane,
                                                     float* __restrict__ part,
                                                     const unsigned char* __restrict__ valid, int ld, long long ps,
                                                     unsigned int* __restrict__ pcnt) {
  __shared__ float xs[SH * SH], ys[SH * SH];
  __shared__ float hs[5][SH * ST];
  __shared__ float red[SN / 64];
  __shared__ unsigned long long vb[MASKED ? (SH * SH + 63) / 64 + 2 : 1];   // void bits of the patch, row-major, zero tail
  __shared__ unsigned long long hb[MASKED ? SH * ST / 64 : 1];              // "a void in the 11 taps right of (r, c)"
  __shared__ unsigned int redc[SN / 64];
  const int plane = blockIdx.y, tile = blockIdx.x;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int q0y = ty * ST, q0x = tx * ST;
  const int i0y = q0y - (SAME ? 5 : 0), i0x = q0x - (SAME ? 5 : 0);
  const long long pbase = MASKED ? (long long)plane * ps : (long long)plane * H * W;
  const int rs = MASKED ? ld : W;
  const float* P = pred + pbase;
  const float* G = gt + pbase;
  if (MASKED && threadIdx.x < 2) vb[(SH * SH + 63) / 64 + threadIdx.x] = 0;
  for (int o = threadIdx.x; o < SH * SH; o += SN) {
    const int r = o / SH, c = o - r * SH;
    const int iy = i0y + r, ix = i0x + c;
    float xv = 0.f, yv = 0.f;
    bool bad = false;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      const long long j = (long long)iy * rs + ix;
      xv = fminf(fmaxf(P[j], 0.f), 1.f);
      yv = G[j];
      if (MASKED) {
        bad = valid && !valid[pbase + j];
        xv = bad ? 0.f : xv;
        yv = bad ? 0.f : yv;
      }
    }
    xs[o] = xv;
    ys[o] = yv;
    if (MASKED) {                                 // lane 0 of a wave holds o = a multiple of 64 and is active whenever a lane is
      const unsigned long long m = __ballot(bad);
      if ((threadIdx.x & 63) == 0) vb[o >> 6] = m;
    }
  }
  __syncthreads();
  // horizontal: SH rows x ST columns of the five moments
  for (int o = threadIdx.x; o < SH * ST; o += SN) {
    const int r = o / ST, c = o - r * ST;
    const float* xr = xs + r * SH + c;
    const float* yr = ys + r * SH + c;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
    for (int t = 0; t < 11; ++t) {
      const float xv = xr[t], yv = yr[t], w = k.w[t];
      a0 += w * xv;
      a1 += w * yv;
      a2 += w * (xv * xv);
      a3 += w * (yv * yv);
      a4 += w * (xv * yv);
    }
    hs[0][o] = a0; hs[1][o] = a1; hs[2][o] = a2; hs[3][o] = a3; hs[4][o] = a4;
    if (MASKED) {                                 // bits p .. p + 10 of the patch; o = r * 32 + c, so a ballot is two rows of hb
      const int p = r * SH + c, wd = p >> 6, sh = p & 63;
      const unsigned long long taps = (vb[wd] >> sh) | (sh ? vb[wd + 1] << (64 - sh) : 0ull);
      const unsigned long long m = __ballot((taps & 0x7FFull) != 0);
      if ((threadIdx.x & 63) == 0) hb[o >> 6] = m;
    }
  }
  __syncthreads();
  // vertical: 4 consecutive rows of one column per thread share 14 staged rows
  const int c = threadIdx.x & (ST - 1), r0 = (threadIdx.x >> 5) * 4;
  unsigned int voids[4] = {0, 0, 0, 0};         // MASKED: nonzero = a void under the window of the thread's element j
  if (MASKED) {
    const unsigned int* hrow = reinterpret_cast<const unsigned int*>(hb);     // 32 columns: one word per row
    unsigned int col = 0;                       // bit t: a void in the 11 taps of row r0 + t from column c on
#pragma unroll
    for (int t = 0; t < 14; ++t) col |= ((hrow[r0 + t] >> c) & 1u) << t;
#pragma unroll
    for (int j = 0; j < 4; ++j) voids[j] = (col >> j) & 0x7FFu;
  }
  float mo[5][4];
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    float v[14];
#pragma unroll
    for (int t = 0; t < 14; ++t) v[t] = hs[m][(r0 + t) * ST + c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < 11; ++t) a += k.w[t] * v[j + t];
      mo[m][j] = a;
    }
  }
  float s_acc = 0.f;
  unsigned int n_acc = 0;
  const int qx = q0x + c;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int qy = q0y + r0 + j;
    if (qy < Hm && qx < Wm) {
      // MASKED: the unmasked arithmetic on every element (same code shape, so the same bits under an all-ones plane); an
      // element with a void under its window is dropped by selects: not summed, not counted, zero coefficients
      const bool counted = !MASKED || voids[j] == 0;
      const float mx = mo[0][j], my = mo[1][j];
      const float sxx = mo[2][j] - mx * mx, syy = mo[3][j] - my * my, sxy = mo[4][j] - mx * my;
      const float A = 2.f * mx * my + C1, B = mx * mx + my * my + C1, Cc = 2.f * sxy + C2, D = sxx + syy + C2;
      const float S = (A * Cc) / (B * D);
      if (MASKED) {
        s_acc = counted ? s_acc + S : s_acc;
        n_acc += counted ? 1u : 0u;
      } else {
        s_acc += S;
      }
      if (!SAME && coef) {
        const long long qi = (long long)plane * Hm * Wm + (long long)qy * Wm + qx;
        const float ca = S * (2.f * my / A - 2.f * mx / B - 2.f * my / Cc + 2.f * mx / D), cb = -S / D, cg = 2.f * S / Cc;
        coef[qi] = counted ? ca : 0.f;
        coef[cplane + qi] = counted ? cb : 0.f;
        coef[2 * cplane + qi] = counted ? cg : 0.f;
      }
    }
  }
  if (MASKED) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n_acc += __shfl_xor(n_acc, d, 64);
    if ((threadIdx.x & 63) == 0) redc[threadIdx.x >> 6] = n_acc;
  }
  s_acc = block_reduce<false>(s_acc, red);
  if (threadIdx.x == 0) {
    part[(size_t)plane * gridDim.x + tile] = s_acc;
    if (MASKED) {
      unsigned int t = 0;
      for (int w = 0; w < SN / 64; ++w) t += redc[w];
      pcnt[(size_t)plane * gridDim.x + tile] = t;
    }
  }
}

// Backward (valid mode) over one ST x ST pixel tile of one plane: the adjoint ("full") window filter of alpha, beta,
// gamma (zero outside the map), then grad[p] += -(w up / M) [Ka + 2 x Kb + y Kg] where 0 <= pred <= 1 (clamp's mask).
// MASKED: cw = (float)(wd / (double)N_s) is formed here from the forward's count (nothing counted: return, the caller's
// zeros stand), and an invalid pixel is skipped -- every window over it has zero coefficients, but pred or gt may hold NaN.
template <bool MASKED>
__global__ __launch_bounds__(SN) void ssim_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const float* __restrict__ coef, long long cplane, int H, int W,
                                                     int Hm, int Wm, int tiles_x, Win11 k,
                                                     const float* __restrict__ gscale, float cw,
                                                     float* __restrict__ grad,
                                                     const unsigned char* __restrict__ valid,
                                                     const long long* __restrict__ ns, double wd) {
  __shared__ float cs[3][SH * SH];
  __shared__ float hs[3][SH * ST];
  if (MASKED) {
    const long long n = ns[0];
    if (n <= 0) return;
    cw = (float)(wd / (double)n);
  }
  const int plane = blockIdx.y, tile = blockIdx.x;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int p0y = ty * ST, p0x = tx * ST;
  const int q0y = p0y - 10, q0x = p0x - 10;          // map elements whose window covers a pixel of the tile
  for (int o = threadIdx.x; o < SH * SH; o += SN) {
    const int r = o / SH, c = o - r * SH;
    const int qy = q0y + r, qx = q0x + c;
    float a = 0.f, b = 0.f, g = 0.f;
    if (qy >= 0 && qy < Hm && qx >= 0 && qx < Wm) {
      const long long qi = (long long)plane * Hm * Wm + (long long)qy * Wm + qx;
      a = coef[qi];
      b = coef[cplane + qi];
      g = coef[2 * cplane + qi];
    }
    cs[0][o] = a; cs[1][o] = b; cs[2][o] = g;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < SH * ST; o += SN) {
    const int r = o / ST, c = o - r * ST;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int t = 0; t < 11; ++t) {          // pixel column c reads map columns c + 10 - t
      const int j = r * SH + c + 10 - t;
      const float w = k.w[t];
      a0 += w * cs[0][j];
      a1 += w * cs[1][j];
      a2 += w * cs[2][j];
    }
    hs[0][o] = a0; hs[1][o] = a1; hs[2][o] = a2;
  }
  __syncthreads();
  const int c = threadIdx.x & (ST - 1), r0 = (threadIdx.x >> 5) * 4;
  float kf[3][4];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    float v[14];
#pragma unroll
    for (int t = 0; t < 14; ++t) v[t] = hs[m][(r0 + t) * ST + c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = 0.f;
#pragma unroll
      for (int t = 0; t < 11; ++t) a += k.w[t] * v[j + 10 - t];
      kf[m][j] = a;
    }
  }
  const float s = -(gscale ? gscale[0] : 1.f) * cw;
  const int px = p0x + c;
  const long long base = (long long)plane * H * W;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int py = p0y + r0 + j;
    if (py < H && px < W) {
      const long long i = base + (long long)py * W + px;
      const float x = pred[i], y = gt[i];
      if (MASKED && !valid[i]) continue;          // the gradient there stays the +0.0 the caller wrote
      if (x >= 0.f && x <= 1.f) grad[i] += s * (kf[0][j] + 2.f * x * kf[1][j] + y * kf[2][j]);
    }
  }
}

// out[k] = term of key k (config order), out[n] = Total = sum_k w_k out[k] (in double over the fp32 values, rounded
// once).  Slots 0..2 come from jspsr_loss_forward's losses[0..2] when the caller passes them.  Every fold is a
// latency-bound walk by one wave, so they run side by side: psum's columns 0..2 by waves 0..2, then ssum (NULL: none
// configured).  Unmasked: 4 waves, the divisors are the host's n and m.  MASKED: 6 waves, wave 3 folds pcnt and wave 5
// scnt between and after them, the divisors are those counts (0: the term is 0), and nn[0] = N, ns[0] = N_s (ns NULL
// without SSIM) are left for the backward.
template <bool MASKED>
__global__ void menu_combine_kernel(const float* __restrict__ psum, const unsigned int* __restrict__ pcnt, int nb,
                                    const float* __restrict__ ssum, const unsigned int* __restrict__ scnt, int nbs,
                                    long long n, long long m, const float* __restrict__ base, KeyMap km,
                                    float* __restrict__ out, long long* __restrict__ nn, long long* __restrict__ ns) {
  __shared__ double acc[4];
  __shared__ long long cnt[2];
  const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (q < 3) {
    const double s = wave_fold(psum, nb, 3, q);
    if (lane == 0) acc[q] = s;
  } else if (q == (MASKED ? 4 : 3)) {
    const double s = wave_fold(ssum, nbs, 1, 0);
    if (lane == 0) acc[3] = s;
  } else if constexpr (MASKED) {
    const long long c = q == 3 ? wave_count(pcnt, nb, 1, 0) : wave_count(scnt, nbs, 1, 0);
    if (lane == 0) cnt[q == 3 ? 0 : 1] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma clang fp contract(off)
    if constexpr (MASKED) { n = cnt[0]; m = cnt[1]; }
    const bool any = !MASKED || n > 0;
    float f[NSLOT];
    for (int i = 0; i < 3; ++i) f[i] = base ? base[i] : 0.f;
    f[S_BERHU] = any ? (float)(acc[0] / (double)n) : 0.f;
    f[S_BCE] = any ? (float)(acc[1] / (double)n) : 0.f;
    f[S_NORM] = any ? (float)(acc[2] / (double)n) : 0.f;
    f[S_SSIM] = m > 0 ? (float)(1.0 - acc[3] / (double)m) : 0.f;
    double tot = 0.0;
    for (int i = 0; i < km.n; ++i) {
      const float v = f[km.slot[i]];
      out[i] = v;
      tot += km.w[i] * (double)v;
    }
    out[km.n] = (float)tot;
    if constexpr (MASKED) {
      nn[0] = n;
      if (ns) ns[0] = m;
    }
  }
}

// out[0] = mean SSIM over every map element of every plane
__global__ void ssim_finalize_kernel(const float* __restrict__ ssum, int nbs, long long m, float* __restrict__ out) {
  const double s = wave_fold(ssum, nbs, 1, 0);
  if (threadIdx.x == 0) out[0] = (float)(s / (double)m);
}

bool dims_ok(int planes, int H, int W) {
  return planes > 0 && H > 0 && W > 0 && planes <= 65535 && (long long)planes * H * W < (1ll << 40);
}

// Per-tile form: workgroup b (one wave) folds plane b's `tiles` partials in ssim_finalize_kernel's order for a
// single-sample call and divides by the plane's own count; a plane with nothing counted is NaN with count 0.
__global__ void ssim_tiles_finalize_kernel(const float* __restrict__ ssum, const unsigned int* __restrict__ scnt, int tiles,
                                           float* __restrict__ out, int* __restrict__ counts) {
  const int b = blockIdx.x;
  const double s = wave_fold(ssum + (size_t)b * tiles, tiles, 1, 0);
  const long long m = wave_count(scnt + (size_t)b * tiles, tiles, 1, 0);
  if (threadIdx.x == 0) {
    out[b] = m > 0 ? (float)(s / (double)m) : __int_as_float(0x7fc00000);
    counts[b] = (int)m;
  }
}

// the forward of one (SAME, MASKED) pair; the arguments are ssim_fwd_kernel's
template <bool MASKED>
void launch_ssim_fwd(bool same, dim3 grid, hipStream_t st, const float* pred, const float* gt, int H, int W, int Hm, int Wm,
                     int tiles_x, const Win11& k, float* coef, long long cplane, float* part, const unsigned char* valid, int ld,
                     long long ps, unsigned int* pcnt) {
  if (same)
    hipLaunchKernelGGL((ssim_fwd_kernel<true, MASKED>), grid, dim3(SN), 0, st, pred, gt, H, W, Hm, Wm, tiles_x, k, coef, cplane,
                       part, valid, ld, ps, pcnt);
  else
    hipLaunchKernelGGL((ssim_fwd_kernel<false, MASKED>), grid, dim3(SN), 0, st, pred, gt, H, W, Hm, Wm, tiles_x, k, coef, cplane,
                       part, valid, ld, ps, pcnt);
}

// ---- the menu's host path ----------------------------------------------------------------------------------------------
// jspsr_loss_menu_* (no plane), jspsr_loss_menu_valid_* (K19: a plane, the SSIM bit refused) and
// jspsr_loss_menu_valid_ssim_* (K23: a plane, SSIM under the "window" rule, ssim_rule 1 -- a map element counts iff every
// pixel under its 11x11 window is valid) are one path.  name: the entry's, for its messages.
struct Family {
  const char* name;
  bool masked, allow_ssim;
  int ssim_rule;            // an entry without the argument passes 1
};

bool menu_query_ok(const Family& f, int terms, int planes, int H, int W) {
  return terms > 0 && !(terms & ~T_ALL) && dims_ok(planes, H, W) && f.ssim_rule == 1 && (f.allow_ssim || !(terms & T_SSIM)) &&
         !((terms & T_SSIM) && (H < 11 || W < 11));
}

// The refusals shared by forward and backward, in every entry's order; ptrs_ok: the caller's own pointer and count checks.
int menu_args_ok(const Family& f, bool ptrs_ok, const unsigned char* valid, int terms, int planes, int H, int W,
                 const void* workspace) {
  if (!ptrs_ok || (f.masked && !valid) || !workspace || terms <= 0 || (terms & ~T_ALL) || !dims_ok(planes, H, W))
    return fail(JSPSR_EINVAL, "%s: bad arguments", f.name);
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "%s: workspace not 16-byte aligned", f.name);
  if (f.ssim_rule != 1) return fail(JSPSR_EINVAL, "%s: ssim_rule %d (1 = window is the rule built)", f.name, f.ssim_rule);
  if ((terms & T_SSIM) && !f.allow_ssim) return fail(JSPSR_EINVAL, "%s: SSIM over a validity plane is not built", f.name);
  if ((terms & T_SSIM) && (H < 11 || W < 11)) return fail(JSPSR_EINVAL, "%s: SSIM needs H, W >= 11", f.name);
  return JSPSR_OK;
}

int menu_forward(const Family& f, const float* pred, const float* gt, const unsigned char* valid, int terms, int planes,
                 int H, int W, int n_keys, const int* key_slot, const double* key_weight, const float* base_losses, float* out,
                 void* workspace, jspsr_stream_t stream) {
  const bool ptrs_ok = pred && gt && out && key_slot && key_weight && n_keys > 0 && n_keys <= MAXKEY;
  if (int e = menu_args_ok(f, ptrs_ok, valid, terms, planes, H, W, workspace)) return e;
  KeyMap km{};
  km.n = n_keys;
  for (int i = 0; i < n_keys; ++i) {
    const int s = key_slot[i];
    const bool ok = (s >= S_L1 && s <= S_GRAD && base_losses) || (s >= S_BERHU && s < NSLOT && (terms & (1 << (s - S_BERHU))));
    if (!ok) return fail(JSPSR_EINVAL, "%s: key %d has slot %d outside the configured terms", f.name, i, s);
    km.slot[i] = s;
    km.w[i] = key_weight[i];
  }
  const bool M = f.masked;
  const Layout L = layout(terms, planes, H, W, M);
  char* ws = static_cast<char*>(workspace);
  auto fl = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
  auto un = [&](size_t off) { return reinterpret_cast<unsigned int*>(ws + off); };
  auto ll = [&](size_t off) { return reinterpret_cast<long long*>(ws + off); };
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long n = (long long)planes * H * W;
  const bool pw = terms & (T_BERHU | T_BCE | T_NORM), ss = terms & T_SSIM;
  if (terms & T_BERHU) {
    if (M) hipLaunchKernelGGL(menu_max_kernel<true>, dim3(L.nbm), dim3(PT), 0, st, pred, gt, valid, n, fl(L.pmax));
    else hipLaunchKernelGGL(menu_max_kernel<false>, dim3(L.nbm), dim3(PT), 0, st, pred, gt, nullptr, n, fl(L.pmax));
    if (int e = check_launch(M ? "loss_menu_valid_max" : "loss_menu_max")) return e;
  }
  if (pw) {
    if (M) hipLaunchKernelGGL(menu_sum_kernel<true>, dim3(L.nb), dim3(PT), 0, st, pred, gt, valid, n, terms, fl(L.pmax), L.nbm,
                              fl(0), fl(L.psum), un(L.pcnt));
    else hipLaunchKernelGGL(menu_sum_kernel<false>, dim3(L.nb), dim3(PT), 0, st, pred, gt, nullptr, n, terms, fl(L.pmax), L.nbm,
                            fl(0), fl(L.psum), nullptr);
    if (int e = check_launch(M ? "loss_menu_valid_sum" : "loss_menu_sum")) return e;
  }
  if (ss) {
    const dim3 grid(L.tiles_x * L.tiles_y, planes);
    if (M) launch_ssim_fwd<true>(false, grid, st, pred, gt, H, W, L.Hm, L.Wm, L.tiles_x, gaussian_window(), fl(L.coef), L.cplane,
                                 fl(L.ssum), valid, W, (long long)H * W, un(L.scnt));
    else launch_ssim_fwd<false>(false, grid, st, pred, gt, H, W, L.Hm, L.Wm, L.tiles_x, gaussian_window(), fl(L.coef), L.cplane,
                                fl(L.ssum), nullptr, 0, 0ll, nullptr);
    if (int e = check_launch(M ? "ssim_valid_forward" : "ssim_forward")) return e;
  }
  const float* psum = pw ? fl(L.psum) : nullptr;
  const float* ssum = ss ? fl(L.ssum) : nullptr;
  if (M)
    hipLaunchKernelGGL(menu_combine_kernel<true>, dim3(1), dim3(6 * 64), 0, st, psum, pw ? un(L.pcnt) : nullptr, L.nb, ssum,
                       ss ? un(L.scnt) : nullptr, L.nbs, 0ll, 0ll, base_losses, km, out, ll(L.nn), ss ? ll(L.ns) : nullptr);
  else
    hipLaunchKernelGGL(menu_combine_kernel<false>, dim3(1), dim3(4 * 64), 0, st, psum, nullptr, L.nb, ssum, nullptr, L.nbs, n,
                       L.cplane, base_losses, km, out, nullptr, nullptr);
  return check_launch(M ? "loss_menu_valid_combine" : "loss_menu_combine");
}

int menu_backward(const Family& f, const float* pred, const float* gt, const unsigned char* valid, int terms, int planes,
                  int H, int W, const double* slot_weight, const float* grad_total, float* grad_pred, const void* workspace,
                  jspsr_stream_t stream) {
  if (int e = menu_args_ok(f, pred && gt && grad_pred && slot_weight, valid, terms, planes, H, W, workspace)) return e;
  const bool M = f.masked;
  const Layout L = layout(terms, planes, H, W, M);
  const char* ws = static_cast<const char*>(workspace);
  const float* th = reinterpret_cast<const float*>(ws);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long n = (long long)planes * H * W;
  const double wb = slot_weight[S_BERHU], wc = slot_weight[S_BCE], wn = slot_weight[S_NORM], wd = slot_weight[S_SSIM];
  if (terms & (T_BERHU | T_BCE | T_NORM)) {
    const double dn = (double)n;
    if (M) hipLaunchKernelGGL(menu_bwd_kernel<true>, dim3(L.nb), dim3(PT), 0, st, pred, gt, valid, n, terms, th,
                              reinterpret_cast<const long long*>(ws + L.nn), grad_total, wb, wc, wn, grad_pred);
    else hipLaunchKernelGGL(menu_bwd_kernel<false>, dim3(L.nb), dim3(PT), 0, st, pred, gt, nullptr, n, terms, th, nullptr,
                            grad_total, (float)(wb / dn), (float)(wc / dn), (float)(wn / (1e-12 * dn)), grad_pred);
    if (int e = check_launch(M ? "loss_menu_valid_backward" : "loss_menu_backward")) return e;
  }
  if (terms & T_SSIM) {
    const int tx = (W + ST - 1) / ST, ty = (H + ST - 1) / ST;
    const float* coef = reinterpret_cast<const float*>(ws + L.coef);
    if (M) hipLaunchKernelGGL(ssim_bwd_kernel<true>, dim3(tx * ty, planes), dim3(SN), 0, st, pred, gt, coef, L.cplane, H, W, L.Hm,
                              L.Wm, tx, gaussian_window(), grad_total, 0.f, grad_pred, valid,
                              reinterpret_cast<const long long*>(ws + L.ns), wd);
    else hipLaunchKernelGGL(ssim_bwd_kernel<false>, dim3(tx * ty, planes), dim3(SN), 0, st, pred, gt, coef, L.cplane, H, W, L.Hm,
                            L.Wm, tx, gaussian_window(), grad_total, (float)(wd / (double)L.cplane), grad_pred, nullptr, nullptr,
                            0.0);
    if (int e = check_launch(M ? "ssim_valid_backward" : "ssim_backward")) return e;
  }
  return JSPSR_OK;
}

}  // namespace

extern "C" size_t jspsr_loss_menu_workspace_bytes(int terms, int planes, int H, int W) {
  return menu_query_ok({"", false, true, 1}, terms, planes, H, W) ? layout(terms, planes, H, W, false).bytes : 0;
}

extern "C" int jspsr_loss_menu_forward(const float* pred, const float* gt, int terms, int planes, int H, int W,
                                       int n_keys, const int* key_slot, const double* key_weight,
                                       const float* base_losses, float* out, void* workspace, jspsr_stream_t stream) {
  return menu_forward({"loss_menu_forward", false, true, 1}, pred, gt, nullptr, terms, planes, H, W, n_keys, key_slot,
                      key_weight, base_losses, out, workspace, stream);
}

extern "C" int jspsr_loss_menu_backward(const float* pred, const float* gt, int terms, int planes, int H, int W,
                                        const double* slot_weight, const float* grad_total, float* grad_pred,
                                        const void* workspace, jspsr_stream_t stream) {
  return menu_backward({"loss_menu_backward", false, true, 1}, pred, gt, nullptr, terms, planes, H, W, slot_weight, grad_total,
                       grad_pred, workspace, stream);
}

// K19: jspsr_loss_menu_valid_ssim_* with the SSIM bit refused
extern "C" size_t jspsr_loss_menu_valid_workspace_bytes(int terms, int planes, int H, int W) {
  return menu_query_ok({"", true, false, 1}, terms, planes, H, W) ? layout(terms, planes, H, W, true).bytes : 0;
}

extern "C" int jspsr_loss_menu_valid_forward(const float* pred, const float* gt, const unsigned char* valid, int terms,
                                             int planes, int H, int W, int n_keys, const int* key_slot,
                                             const double* key_weight, const float* base_losses, float* out, void* workspace,
                                             jspsr_stream_t stream) {
  return menu_forward({"loss_menu_valid_forward", true, false, 1}, pred, gt, valid, terms, planes, H, W, n_keys, key_slot,
                      key_weight, base_losses, out, workspace, stream);
}

extern "C" int jspsr_loss_menu_valid_backward(const float* pred, const float* gt, const unsigned char* valid, int terms,
                                              int planes, int H, int W, const double* slot_weight, const float* grad_total,
                                              float* grad_pred, const void* workspace, jspsr_stream_t stream) {
  return menu_backward({"loss_menu_valid_backward", true, false, 1}, pred, gt, valid, terms, planes, H, W, slot_weight,
                       grad_total, grad_pred, workspace, stream);
}

// K23: the plane and SSIM under ssim_rule (1 = window)
extern "C" size_t jspsr_loss_menu_valid_ssim_workspace_bytes(int terms, int planes, int H, int W, int ssim_rule) {
  return menu_query_ok({"", true, true, ssim_rule}, terms, planes, H, W) ? layout(terms, planes, H, W, true).bytes : 0;
}

extern "C" int jspsr_loss_menu_valid_ssim_forward(const float* pred, const float* gt, const unsigned char* valid, int terms,
                                                  int planes, int H, int W, int ssim_rule, int n_keys, const int* key_slot,
                                                  const double* key_weight, const float* base_losses, float* out,
                                                  void* workspace, jspsr_stream_t stream) {
  return menu_forward({"loss_menu_valid_ssim_forward", true, true, ssim_rule}, pred, gt, valid, terms, planes, H, W, n_keys,
                      key_slot, key_weight, base_losses, out, workspace, stream);
}

extern "C" int jspsr_loss_menu_valid_ssim_backward(const float* pred, const float* gt, const unsigned char* valid, int terms,
                                                   int planes, int H, int W, int ssim_rule, const double* slot_weight,
                                                   const float* grad_total, float* grad_pred, const void* workspace,
                                                   jspsr_stream_t stream) {
  return menu_backward({"loss_menu_valid_ssim_backward", true, true, ssim_rule}, pred, gt, valid, terms, planes, H, W,
                       slot_weight, grad_total, grad_pred, workspace, stream);
}

extern "C" size_t jspsr_ssim_workspace_bytes(int planes, int H, int W, int same) {
  if (!dims_ok(planes, H, W) || (!same && (H < 11 || W < 11))) return 0;
  const int Hm = same ? H : H - 10, Wm = same ? W : W - 10;
  return al16((size_t)((Wm + ST - 1) / ST) * ((Hm + ST - 1) / ST) * planes * 4);
}

extern "C" int jspsr_ssim_forward(const float* pred, const float* gt, int planes, int H, int W, int same,
                                  const float* window11, float* out, void* workspace, jspsr_stream_t stream) {
  if (!pred || !gt || !out || !workspace || !dims_ok(planes, H, W)) return fail(JSPSR_EINVAL, "ssim_forward: bad arguments");
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "ssim_forward: workspace not 16-byte aligned");
  if (!same && (H < 11 || W < 11)) return fail(JSPSR_EINVAL, "ssim_forward: valid mode needs H, W >= 11");
  Win11 k = gaussian_window();
  if (window11)
    for (int i = 0; i < 11; ++i) k.w[i] = window11[i];
  const int Hm = same ? H : H - 10, Wm = same ? W : W - 10;
  const int tx = (Wm + ST - 1) / ST, ty = (Hm + ST - 1) / ST;
  float* part = static_cast<float*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  launch_ssim_fwd<false>(same, dim3(tx * ty, planes), st, pred, gt, H, W, Hm, Wm, tx, k, nullptr, 0ll, part, nullptr, 0, 0ll, nullptr);
  if (int e = check_launch("ssim_forward")) return e;
  hipLaunchKernelGGL(ssim_finalize_kernel, dim3(1), dim3(64), 0, st, part, tx * ty * planes, (long long)planes * Hm * Wm, out);
  return check_launch("ssim_finalize");
}

// Per-tile SSIM of a batch of uncropped (B,1,H,W) tiles: the crop of `border` on every side (int(H * border) rows,
// int(W * border) columns, as metrics.prepare) by index arithmetic, one forward launch over (tiles of the map, B) and a
// finalize: out[b] = the mean over tile b's counted map elements (NaN where none), counts[b] = their number.
extern "C" size_t jspsr_ssim_tiles_workspace_bytes(int B, int H, int W, double border, int same) {
  if (!(border >= 0.0) || border >= 0.5 || !dims_ok(B, H, W)) return 0;
  const int h = H - 2 * (int)((double)H * border), w = W - 2 * (int)((double)W * border);
  if (h <= 0 || w <= 0 || (!same && (h < 11 || w < 11))) return 0;
  const int Hm = same ? h : h - 10, Wm = same ? w : w - 10;
  return 2 * al16((size_t)((Wm + ST - 1) / ST) * ((Hm + ST - 1) / ST) * B * 4);
}

extern "C" int jspsr_ssim_tiles_forward(const float* pred, const float* gt, const unsigned char* valid, int B, int H, int W,
                                        double border, int same, const float* window11, float* out, int* counts,
                                        void* workspace, jspsr_stream_t stream) {
  if (!pred || !gt || !out || !counts || !workspace || !dims_ok(B, H, W))
    return fail(JSPSR_EINVAL, "ssim_tiles_forward: bad arguments");
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "ssim_tiles_forward: workspace not 16-byte aligned");
  if (!(border >= 0.0) || border >= 0.5) return fail(JSPSR_EINVAL, "ssim_tiles_forward: border must be in [0, 0.5)");
  const int bh = (int)((double)H * border), bw = (int)((double)W * border);       // int(h * border), metrics.prepare
  const int h = H - 2 * bh, w = W - 2 * bw;
  if (h <= 0 || w <= 0) return fail(JSPSR_EINVAL, "ssim_tiles_forward: nothing left after the border crop");
  if (!same && (h < 11 || w < 11)) return fail(JSPSR_EINVAL, "ssim_tiles_forward: valid mode needs H, W >= 11 after the crop");
  Win11 k = gaussian_window();
  if (same && window11)
    for (int i = 0; i < 11; ++i) k.w[i] = window11[i];
  const int Hm = same ? h : h - 10, Wm = same ? w : w - 10;
  const int tx = (Wm + ST - 1) / ST, ty = (Hm + ST - 1) / ST;
  const size_t half = al16((size_t)tx * ty * B * 4);
  float* part = static_cast<float*>(workspace);
  unsigned int* pcnt = reinterpret_cast<unsigned int*>(static_cast<char*>(workspace) + half);
  const long long o = (long long)bh * W + bw;
  hipStream_t st = static_cast<hipStream_t>(stream);
  launch_ssim_fwd<true>(same, dim3(tx * ty, B), st, pred + o, gt + o, h, w, Hm, Wm, tx, k, nullptr, 0ll, part,
                        valid ? valid + o : nullptr, W, (long long)H * W, pcnt);
  if (int e = check_launch("ssim_tiles_forward")) return e;
  hipLaunchKernelGGL(ssim_tiles_finalize_kernel, dim3(B), dim3(64), 0, st, part, pcnt, tx * ty, out, counts);
  return check_launch("ssim_tiles_finalize");
}
