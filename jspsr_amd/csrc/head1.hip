// K1p -- the plain output head of JSPSR(spn=False) and EDSR(spn=False): one nn.Conv2d(C, 1, 3, padding=1) on the last
// feature (reference models/JSPSR.py:195-204,378: Basic2d(c0_channels, 1, 3, bn=False, relu=False); models/EDSR.py:
// 108-111,132-136: self.head), and its autograd.  The head reads C values per pixel and writes 4 bytes: it is HBM-bound,
// so it runs on the vector ALUs in fp32 (bf16 inputs widened exactly) and writes the fp32 prediction planes directly --
// no GEMM padding of the one output channel, no NHWC -> NCHW pass, and the prediction is never rounded to bf16.
//
//   forward   thread = one output column of a band of ROWS rows; it streams the band's input rows y0-1 .. y0+ROWS once,
//             reading its pixel and its two horizontal neighbours (those come from L1: the neighbouring lanes read the same
//             lines) and folding each input row into three rolling row accumulators (taps ky = 2, 1, 0).  Every output
//             sums its 9 x C products in a fixed order: ky = 0, 1, 2, then kx = 0, 1, 2, then channel.
//   backward  workgroup = a TROWS x TCOLS pixel tile; the tile's dy (with a one-pixel halo, zeros outside the image) is
//             staged in LDS once.  Lane = (pixel, 8-channel chunk), so that a wave's loads and stores of x / dx cover
//             contiguous NHWC bytes; each lane keeps its chunk's 8 x 9 weight-gradient sums in registers and writes dx of
//             its chunk (w^T dy, fixed tap order).  The workgroup's sums are reduced in a fixed order through LDS into one
//             partial row per workgroup; a second launch folds the rows in a fixed order (fp64), so dW / db are the same
//             bits from run to run.
#include "common.h"

namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int FROWS = 8;                 // forward: output rows per workgroup
constexpr int TROWS = 32, TCOLS = 64;    // backward: pixel tile per workgroup
constexpr int BWAVES = 4;                // backward: waves per workgroup
constexpr int FOLD_GROUPS = 16;          // fold: partial rows summed side by side per entry

struct Head1Args {
  const void* x;       // (B,H,W,x_cs) NHWC, first channel x_coff
  const float* w;      // [C][3][3] fp32 (nn.Conv2d layout)
  const float* bias;   // [1]
  float* y;            // forward: (B,1,H,W) fp32
  const float* dy;     // backward: (B,1,H,W) fp32
  void* dx;            // backward: (B,H,W,dx_cs) NHWC, first channel dx_coff; NULL = not wanted
  float* partial;      // backward: [workgroups][9 C + 1]
  int x_cs, x_coff, dx_cs, dx_coff, C, H, W;
};

__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ unsigned bf16_bits(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }  // RNE

// 8 consecutive channels at p (16-byte aligned) -> fp32
template <typename T>
__device__ __forceinline__ void load8(const T* p, float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    const u32x4 u = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = bf16_lo(u[i]); v[2 * i + 1] = bf16_hi(u[i]); }
  } else {
    const u32x4 a = reinterpret_cast<const u32x4*>(p)[0], b = reinterpret_cast<const u32x4*>(p)[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = __uint_as_float(a[i]); v[4 + i] = __uint_as_float(b[i]); }
  }
}

template <typename T>
__device__ __forceinline__ void store8(T* p, const float (&v)[8]) {
  if constexpr (sizeof(T) == 2) {
    u32x4 u;
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = bf16_bits(v[2 * i]) | (bf16_bits(v[2 * i + 1]) << 16);
    *reinterpret_cast<u32x4*>(p) = u;
  } else {
    u32x4 a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) { a[i] = __float_as_uint(v[i]); b[i] = __float_as_uint(v[4 + i]); }
    reinterpret_cast<u32x4*>(p)[0] = a;
    reinterpret_cast<u32x4*>(p)[1] = b;
  }
}

// ---- forward ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void head1_fwd_kernel(const Head1Args A) {
  const int xo = blockIdx.x * blockDim.x + threadIdx.x;
  const int y0 = blockIdx.y * FROWS, b = blockIdx.z;
  const int y_end = min(y0 + FROWS, A.H);
  const bool col_ok = xo < A.W;
  const T* xb = static_cast<const T*>(A.x) + (size_t)b * A.H * A.W * A.x_cs + A.x_coff;
  // weights as (w[c][0][kx], w[c][1][kx], w[c][2][kx], 0): one broadcast 16-byte LDS read per channel and column tap
  __shared__ f32x4 w_s[3][256];
  for (int i = threadIdx.x; i < 3 * A.C; i += blockDim.x) {
    const int kx = i / A.C, c = i % A.C;
    const float* wc = A.w + c * 9 + kx;
    w_s[kx][c] = f32x4{wc[0], wc[3], wc[6], 0.f};
  }
  __syncthreads();
  float a_prev = 0.f, a_cur = 0.f, a_next = 0.f;       // output rows y-1, y, y+1 while input row y streams
  for (int y = y0 - 1; y <= y_end; ++y) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;                // taps ky = 0 (-> output y+1), 1 (-> y), 2 (-> y-1)
    if (col_ok && y >= 0 && y < A.H) {
      const T* row = xb + (size_t)y * A.W * A.x_cs;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xi = xo + kx - 1;
        if (xi < 0 || xi >= A.W) continue;
        const T* px = row + (size_t)xi * A.x_cs;
        const f32x4* wk = w_s[kx];
#pragma unroll 4
        for (int c = 0; c < A.C; c += 8) {
          float v[8];
          load8(px + c, v);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const f32x4 q = wk[c + i];
            s0 = __builtin_fmaf(v[i], q.x, s0);
            s1 = __builtin_fmaf(v[i], q.y, s1);
            s2 = __builtin_fmaf(v[i], q.z, s2);
          }
        }
      }
    }
    a_prev += s2;
    a_cur += s1;
    a_next += s0;
    if (col_ok && y - 1 >= y0) A.y[((size_t)b * A.H + (y - 1)) * A.W + xo] = a_prev + A.bias[0];
    a_prev = a_cur;
    a_cur = a_next;
    a_next = 0.f;
  }
}

// ---- backward ---------------------------------------------------------------------------------------------------------
template <typename T, bool WANT_DX>
__global__ __launch_bounds__(BWAVES * 64) void head1_bwd_kernel(const Head1Args A) {
  __shared__ float g_s[TROWS + 2][TCOLS + 2];          // dy of the tile, one-pixel halo, zeros outside the image
  __shared__ float red[BWAVES * 64][9];                // cross-lane reduction, 8 sums per lane per round (+1 pad)
  const int tiles_x = (A.W + TCOLS - 1) / TCOLS, tiles_y = (A.H + TROWS - 1) / TROWS;
  const int wg = blockIdx.x;
  const int b = wg / (tiles_x * tiles_y), t = wg % (tiles_x * tiles_y);
  const int y0 = (t / tiles_x) * TROWS, x0 = (t % tiles_x) * TCOLS;
  const float* dyb = A.dy + (size_t)b * A.H * A.W;
  for (int i = threadIdx.x; i < (TROWS + 2) * (TCOLS + 2); i += blockDim.x) {
    const int r = i / (TCOLS + 2), c = i % (TCOLS + 2), yy = y0 + r - 1, xx = x0 + c - 1;
    g_s[r][c] = (yy >= 0 && yy < A.H && xx >= 0 && xx < A.W) ? dyb[(size_t)yy * A.W + xx] : 0.f;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = A.C >> 3, ppw = 64 / nch;            // 8-channel chunks per pixel, pixels per wave step
  const int pp = lane / nch, ch = lane % nch;
  const bool active = pp < ppw;
  float wv[8][9];                                      // this lane's chunk of the weights
  float acc[8][9];                                     // ... and of the weight gradient
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      wv[i][k] = active ? A.w[(ch * 8 + i) * 9 + k] : 0.f;
      acc[i][k] = 0.f;
    }
  const T* xb = static_cast<const T*>(A.x) + (size_t)b * A.H * A.W * A.x_cs + A.x_coff + ch * 8;
  T* dxb = WANT_DX ? static_cast<T*>(A.dx) + (size_t)b * A.H * A.W * A.dx_cs + A.dx_coff + ch * 8 : nullptr;
  const int step = BWAVES * ppw;
  if (active) {
#pragma unroll 2
    for (int i = wave * ppw + pp; i < TROWS * TCOLS; i += step) {
      const int ty = i / TCOLS, tx = i % TCOLS, yy = y0 + ty, xx = x0 + tx;
      if (yy >= A.H || xx >= A.W) continue;
      float g[9];                                      // g[ky*3+kx] = dy(yy - ky + 1, xx - kx + 1)
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) g[ky * 3 + kx] = g_s[ty - ky + 2][tx - kx + 2];
      const size_t pix = (size_t)yy * A.W + xx;
      float v[8];
      load8(xb + pix * A.x_cs, v);
#pragma unroll
      for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[c][k] = __builtin_fmaf(v[c], g[k], acc[c][k]);
      if constexpr (WANT_DX) {
        float d[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          float s = 0.f;
#pragma unroll
          for (int k = 0; k < 9; ++k) s = __builtin_fmaf(wv[c][k], g[k], s);
          d[c] = s;
        }
        store8(dxb + pix * A.dx_cs, d);
      }
    }
  }

  // workgroup sums, fixed order: round r moves the lanes' sums j = 8 r .. 8 r + 7 (j = 9 c + k) through LDS; thread
  // (chunk, jj) adds the lanes of its chunk in wave / pixel order
  float* out = A.partial + (size_t)wg * (9 * A.C + 1);
  const float* accf = &acc[0][0];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) red[threadIdx.x][jj] = accf[8 * r + jj];
    __syncthreads();
    if ((int)threadIdx.x < nch * 8) {
      const int c = threadIdx.x >> 3, jj = threadIdx.x & 7;
      float s = 0.f;
      for (int w = 0; w < BWAVES; ++w)
        for (int q = 0; q < ppw; ++q) s += red[w * 64 + q * nch + c][jj];
      out[c * 72 + 8 * r + jj] = s;
    }
    __syncthreads();
  }
  if (threadIdx.x < 64) {                              // bias gradient: the tile's dy, column by column, then across lanes
    float s = 0.f;
    for (int r = 0; r < TROWS; ++r) s += g_s[r + 1][threadIdx.x + 1];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (threadIdx.x == 0) out[9 * A.C] = s;
  }
}

// entry e of the 9 C + 1 gradient values = sum over the workgroups' partial rows: FOLD_GROUPS strided sums, then their sum,
// all in a fixed order
__global__ __launch_bounds__(64 * FOLD_GROUPS) void head1_fold_kernel(const float* partial, int rows, int n, float* dw, float* db) {
  __shared__ double s_part[FOLD_GROUPS][64];
  const int e = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
  double s = 0.0;
  if (e < n)
    for (int r = grp; r < rows; r += FOLD_GROUPS) s += (double)partial[(size_t)r * n + e];
  s_part[grp][threadIdx.x & 63] = s;
  __syncthreads();
  if (grp == 0 && e < n) {
    double t = 0.0;
    for (int g = 0; g < FOLD_GROUPS; ++g) t += s_part[g][threadIdx.x];
    if (e < n - 1) dw[e] = (float)t;
    else db[0] = (float)t;
  }
}

bool c_ok(int C) { return C > 0 && C <= 256 && C % 8 == 0; }

int check_tensor(const char* who, int dtype, int C, int cs, int coff, const void* p, const char* name) {
  const int e = dtype == JSPSR_BF16 ? 8 : 4;
  if (cs < coff + C || coff < 0 || cs % e || coff % e)
    return jspsr::fail(JSPSR_EINVAL, "%s: %s channel pitch %d / offset %d (C %d; 16-byte chunks)", who, name, cs, coff, C);
  if (!jspsr::aligned16(p)) return jspsr::fail(JSPSR_EALIGN, "%s: %s not 16-byte aligned", who, name);
  return JSPSR_OK;
}

int check_common(const char* who, int dtype, int C, int B, int H, int W) {
  if (dtype != JSPSR_F32 && dtype != JSPSR_BF16) return jspsr::fail(JSPSR_EINVAL, "%s: bad dtype %d", who, dtype);
  if (!c_ok(C)) return jspsr::fail(JSPSR_EINVAL, "%s: C = %d (a multiple of 8, at most 256)", who, C);
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || (long long)H * W >= (1LL << 31))
    return jspsr::fail(JSPSR_EINVAL, "%s: bad shape B %d H %d W %d", who, B, H, W);
  return JSPSR_OK;
}

long long bwd_workgroups(int B, int H, int W) {
  return (long long)B * ((H + TROWS - 1) / TROWS) * ((W + TCOLS - 1) / TCOLS);
}

}  // namespace

extern "C" int jspsr_conv_head1_forward(int dtype, const void* x, int x_cstride, int x_coff, int C, const float* w,
                                        const float* bias, float* y, int B, int H, int W, jspsr_stream_t stream) {
  if (!x || !w || !bias || !y) return jspsr::fail(JSPSR_EINVAL, "conv_head1_forward: null pointer");
  if (int e = check_common("conv_head1_forward", dtype, C, B, H, W)) return e;
  if (int e = check_tensor("conv_head1_forward", dtype, C, x_cstride, x_coff, x, "x")) return e;
  if (!jspsr::aligned4(y) || !jspsr::aligned4(w) || !jspsr::aligned4(bias)) return jspsr::fail(JSPSR_EALIGN, "conv_head1_forward: alignment");
  Head1Args A{};
  A.x = x; A.w = w; A.bias = bias; A.y = y; A.x_cs = x_cstride; A.x_coff = x_coff; A.C = C; A.H = H; A.W = W;
  const int threads = 64 * (W >= 256 ? 4 : (W + 63) / 64);
  const dim3 grid((W + threads - 1) / threads, (H + FROWS - 1) / FROWS, B), block(threads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == JSPSR_BF16) hipLaunchKernelGGL(head1_fwd_kernel<__bf16>, grid, block, 0, s, A);
  else hipLaunchKernelGGL(head1_fwd_kernel<float>, grid, block, 0, s, A);
  return jspsr::check_launch("head1_forward");
}

extern "C" size_t jspsr_conv_head1_workspace_bytes(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || !c_ok(C)) return 0;
  return (size_t)bwd_workgroups(B, H, W) * (9 * C + 1) * sizeof(float);
}

extern "C" int jspsr_conv_head1_backward(int dtype, const float* dy, const void* x, int x_cstride, int x_coff, int C,
                                         const float* w, void* dx, int dx_cstride, int dx_coff, float* dw, float* db,
                                         void* workspace, int B, int H, int W, jspsr_stream_t stream) {
  if (!dy || !x || !w || !dw || !db || !workspace) return jspsr::fail(JSPSR_EINVAL, "conv_head1_backward: null pointer");
  if (int e = check_common("conv_head1_backward", dtype, C, B, H, W)) return e;
  if (int e = check_tensor("conv_head1_backward", dtype, C, x_cstride, x_coff, x, "x")) return e;
  if (dx) {
    if (int e = check_tensor("conv_head1_backward", dtype, C, dx_cstride, dx_coff, dx, "dx")) return e;
  }
  if (!jspsr::aligned4(dy) || !jspsr::aligned4(w) || !jspsr::aligned4(dw) || !jspsr::aligned4(db) || !jspsr::aligned16(workspace))
    return jspsr::fail(JSPSR_EALIGN, "conv_head1_backward: alignment");
  const long long rows = bwd_workgroups(B, H, W);
  if (rows > (1LL << 30)) return jspsr::fail(JSPSR_EINVAL, "conv_head1_backward: too many tiles");
  Head1Args A{};
  A.dy = dy; A.x = x; A.x_cs = x_cstride; A.x_coff = x_coff; A.w = w; A.dx = dx; A.dx_cs = dx_cstride; A.dx_coff = dx_coff;
  A.partial = static_cast<float*>(workspace); A.C = C; A.H = H; A.W = W;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)rows), block(BWAVES * 64);
  if (dtype == JSPSR_BF16) {
    if (dx) hipLaunchKernelGGL((head1_bwd_kernel<__bf16, true>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((head1_bwd_kernel<__bf16, false>), grid, block, 0, s, A);
  } else {
    if (dx) hipLaunchKernelGGL((head1_bwd_kernel<float, true>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((head1_bwd_kernel<float, false>), grid, block, 0, s, A);
  }
  if (int e = jspsr::check_launch("head1_backward")) return e;
  const int n = 9 * C + 1;
  hipLaunchKernelGGL(head1_fold_kernel, dim3((n + 63) / 64), dim3(64 * FOLD_GROUPS), 0, s, A.partial, (int)rows, n, dw, db);
  return jspsr::check_launch("head1_backward_fold");
}
