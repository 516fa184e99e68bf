// The two ends of the training step that touch every pixel / every parameter exactly once:
//   * fused L1 + L2 + Sobel-L1 loss, forward and gradient (reference: MultiLoss, losses/loss_schemes.py:
//     55-72 with configs/*.yml:67-70; EdgeLoss = L1 between kornia spatial_gradient(sobel, normalised)
//     of prediction and target, losses/loss_functions.py:171-185).  The Sobel operator is linear, so the
//     edge term is computed on d = pred - gt; replicate padding is a clamp of the neighbour index.
//   * fused multi-tensor AdamW over one flat parameter/gradient buffer (torch.optim.AdamW semantics,
//     utils/common_config.py:241-291, configs/*.yml:71-76): HBM-bound, 16 B read + 12 B written per
//     parameter.
#include "common.h"
#include "loss_fold.h"

namespace {

using namespace jspsr;

constexpr int LT = 256;

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// The three loss kernels take MASKED (K19): the same loss over the elements a validity plane keeps.  valid: one byte per
// element of pred, nonzero = valid.  One body per pass, so an all-ones plane gives the unmasked bits.  pred / gt at an
// invalid element are read only behind a select (never multiplied by the mask: NaN * 0 is NaN).  A Sobel output is
// counted iff its nine replicate-clamped taps are valid; an uncounted output stores sign bytes 0, which is all the adjoint
// loop needs.  N (valid elements) and N_g (counted outputs) are counted as integers per workgroup, folded by the finalize
// kernel and left in the workspace for the backward: no host round trip.

// pass 1: per-pixel d, Sobel of d, partial sums {sum|d|, sum d^2, sum(|gx|+|gy|)}, signs of gx, gy; MASKED: pcnt {N, N_g}
template <bool MASKED>
__global__ __launch_bounds__(LT) void loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const unsigned char* __restrict__ valid,
                                                     signed char* __restrict__ sg, float* __restrict__ partial,
                                                     unsigned int* __restrict__ pcnt, int B, int H, int W) {
  __shared__ float red[3 * (LT / 64)];
  __shared__ unsigned int redc[MASKED ? 2 * (LT / 64) : 1];
  const long long n = (long long)B * H * W;
  float s[3] = {0.f, 0.f, 0.f};
  unsigned int cnt[2] = {0, 0};
  for (long long i = blockIdx.x * (long long)LT + threadIdx.x; i < n; i += (long long)gridDim.x * LT) {
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const long long base = i - (long long)y * W - x;
    const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
    const int xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
    bool all = true;
    auto D = [&](int yy, int xx) {
      const long long j = base + (long long)yy * W + xx;
      const float dj = pred[j] - gt[j];               // MASKED: loaded beside the plane's byte, not after it
      if constexpr (MASKED) {
        const bool vj = valid[j] != 0;
        all = all && vj;
        return vj ? dj : 0.f;
      } else {
        return dj;
      }
    };
    const float d = D(y, x);                          // 0 at an invalid element: the sums keep their bits
    const bool v = all;
    const float a = D(ym, xm), b = D(ym, x), c = D(ym, xp), e = D(y, xm), f = D(y, xp), g = D(yp, xm), h = D(yp, x), k = D(yp, xp);
    const float gx = ((c - a) + 2.f * (f - e) + (k - g)) * 0.125f;
    const float gy = ((g - a) + 2.f * (h - b) + (k - c)) * 0.125f;
    s[0] += fabsf(d);
    {
#pragma clang fp contract(off)                        // a product and a sum
      s[1] += d * d;
    }
    if constexpr (MASKED) {
      cnt[0] += v ? 1u : 0u;
      if (all) {
        s[2] += fabsf(gx) + fabsf(gy);
        ++cnt[1];
      }
      sg[2 * i] = all ? (signed char)sgn(gx) : (signed char)0;
      sg[2 * i + 1] = all ? (signed char)sgn(gy) : (signed char)0;
    } else {
      s[2] += fabsf(gx) + fabsf(gy);
      sg[2 * i] = (signed char)sgn(gx);
      sg[2 * i + 1] = (signed char)sgn(gy);
    }
  }
  block_fold3<LT, MASKED ? 2 : 0>(s, cnt, red, redc, partial, pcnt);
}

// losses[0..3] = {L1, L2, Grad, Total}.  MASKED: two more waves fold the counts, nn[0..1] = {N, N_g}, and an empty mask
// gives 0, not 0 / 0; else both divisors are the host's n.
template <bool MASKED>
__global__ void loss_finalize_kernel(const float* __restrict__ partial, const unsigned int* __restrict__ pcnt, int rows,
                                     long long n, float w1, float w2, float wg, float* __restrict__ losses,
                                     long long* __restrict__ nn) {
  __shared__ double acc[3];
  __shared__ long long cnt[2];
  const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (q < 3) {
    const double s = wave_fold(partial, rows, 3, q);
    if (lane == 0) acc[q] = s;
  } else if constexpr (MASKED) {
    const long long s = wave_count(pcnt, rows, 2, q - 3);
    if (lane == 0) cnt[q - 3] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long m = n;
    if constexpr (MASKED) { n = cnt[0]; m = cnt[1]; }
    const bool any = !MASKED || n > 0, any_g = !MASKED || m > 0;
    const double l1 = any ? acc[0] / (double)n : 0.0, l2 = any ? acc[1] / (double)n : 0.0;
    const double lg = any_g ? acc[2] / (2.0 * (double)m) : 0.0;
    losses[0] = (float)l1; losses[1] = (float)l2; losses[2] = (float)lg;
    losses[3] = (float)(w1 * l1 + w2 * l2 + wg * lg);
    if constexpr (MASKED) { nn[0] = n; nn[1] = m; }
  }
}

// pass 2: d(Total)/d(pred) * upstream scalar gradient.  Adjoint of the replicate-padded Sobel: pixel p
// collects k[delta] * sign(g[q]) from every (q, delta) with clamp(q + delta) == p.  MASKED: N and N_g are loaded from
// nn, and every invalid element gets +0.0.
template <bool MASKED>
__global__ __launch_bounds__(LT) void loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                     const unsigned char* __restrict__ valid,
                                                     const signed char* __restrict__ sg, const long long* __restrict__ nn,
                                                     const float* __restrict__ gscale, float w1, float w2, float wg,
                                                     float* __restrict__ gpred, int B, int H, int W) {
  const long long n = (long long)B * H * W;
  long long nv = n, ngv = n;
  if constexpr (MASKED) { nv = nn[0]; ngv = nn[1]; }
  const float up = gscale ? gscale[0] : 1.f;
  const bool any = !MASKED || nv > 0, any_g = !MASKED || ngv > 0;       // a count of 0: coefficient 0, not a division
  const float c1 = any ? up * w1 / (float)nv : 0.f, c2 = any ? up * 2.f * w2 / (float)nv : 0.f;
  const float cg = any_g ? up * wg / (2.f * (float)ngv) * 0.125f : 0.f;
  // kernels: gx weight kx[dy][dx] = {-1,0,1; -2,0,2; -1,0,1}, gy weight = its transpose
  for (long long i = blockIdx.x * (long long)LT + threadIdx.x; i < n; i += (long long)gridDim.x * LT) {
    if constexpr (MASKED) {
      if (!valid[i]) {
        gpred[i] = 0.f;
        continue;
      }
    }
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const long long base = i - (long long)y * W - x;
    const float d = pred[i] - gt[i];
    float acc = 0.f;
    for (int qy = y - 1; qy <= y + 1; ++qy) {
      if (qy < 0 || qy >= H) continue;
      for (int qx = x - 1; qx <= x + 1; ++qx) {
        if (qx < 0 || qx >= W) continue;
        const long long j = base + (long long)qy * W + qx;
        const float sx = (float)sg[2 * j], sy = (float)sg[2 * j + 1];
        if (sx == 0.f && sy == 0.f) continue;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          int ty = qy + dy; ty = ty < 0 ? 0 : (ty > H - 1 ? H - 1 : ty);
          if (ty != y) continue;
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            int tx = qx + dx; tx = tx < 0 ? 0 : (tx > W - 1 ? W - 1 : tx);
            if (tx != x) continue;
            const float kx = (float)dx * (dy == 0 ? 2.f : 1.f);
            const float ky = (float)dy * (dx == 0 ? 2.f : 1.f);
            acc += kx * sx + ky * sy;
          }
        }
      }
    }
    // c1 sgn(d) + c2 d + cg acc in stated roundings: both products rounded, their sum rounded, then one fused
    // multiply-add of the Sobel part
    float gv;
    {
#pragma clang fp contract(off)
      const float t = c1 * sgn(d), u = c2 * d;
      gv = __builtin_fmaf(cg, acc, t + u);
    }
    gpred[i] = gv;
  }
}

// AdamW, decoupled weight decay, bias-corrected (torch.optim.AdamW, maximize=False, amsgrad=False)
__device__ __forceinline__ void adamw_one(float& P, float G, float& M, float& V, float lr, float beta1, float beta2,
                                          float eps, float wd, float bc1, float bc2s) {
  P *= 1.f - lr * wd;
  M = beta1 * M + (1.f - beta1) * G;
  V = beta2 * V + (1.f - beta2) * G * G;
  P -= (lr / bc1) * M / (sqrtf(V) / bc2s + eps);
}

// `head` scalar elements bring the four (equally misaligned) buffers to a 16-byte boundary, then float4s, then a tail.
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long n, int head,
                                                   float lr, float beta1, float beta2, float eps, float wd, float bc1,
                                                   float bc2s) {
  const long long n4 = (n - head) / 4;
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* m4 = reinterpret_cast<float4*>(m + head);
  float4* v4 = reinterpret_cast<float4*>(v + head);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 P = p4[i];
    const float4 G = g4[i];
    float4 M = m4[i], V = v4[i];
    adamw_one(P.x, G.x, M.x, V.x, lr, beta1, beta2, eps, wd, bc1, bc2s);
    adamw_one(P.y, G.y, M.y, V.y, lr, beta1, beta2, eps, wd, bc1, bc2s);
    adamw_one(P.z, G.z, M.z, V.z, lr, beta1, beta2, eps, wd, bc1, bc2s);
    adamw_one(P.w, G.w, M.w, V.w, lr, beta1, beta2, eps, wd, bc1, bc2s);
    p4[i] = P;
    m4[i] = M;
    v4[i] = V;
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {  // up to 3 head + 3 tail elements
    const int tail = (int)(n - head - n4 * 4);
    long long i = -1;
    if ((int)threadIdx.x < head) i = threadIdx.x;
    else if ((int)threadIdx.x >= 4 && (int)threadIdx.x - 4 < tail) i = head + n4 * 4 + (threadIdx.x - 4);
    if (i >= 0) {
      float P = p[i], M = m[i], V = v[i];
      adamw_one(P, g[i], M, V, lr, beta1, beta2, eps, wd, bc1, bc2s);
      p[i] = P; m[i] = M; v[i] = V;
    }
  }
}

// The same update with its seven scalars -- lr, beta1, beta2, eps, weight decay, the two bias corrections -- read from DEVICE
// memory: a launch captured in a hipGraph carries its kernel arguments verbatim, and the learning rate and the bias
// corrections change from step to step (jspsr_adamw_step_dev; the caller refreshes the seven floats before every replay).
__global__ __launch_bounds__(256) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v, long long n, int head,
                                                       const float* __restrict__ hyper) {
  const float lr = hyper[0], beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3], wd = hyper[4], bc1 = hyper[5], bc2s = hyper[6];
  const long long n4 = (n - head) / 4;
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* m4 = reinterpret_cast<float4*>(m + head);
  float4* v4 = reinterpret_cast<float4*>(v + head);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    float4 P = p4[i];
    const float4 G = g4[i];
    float4 M = m4[i], V = v4[i];
    adamw_one(P.x, G.x, M.x, V.x, lr, beta1, beta2, eps, wd, bc1, bc2s);
    adamw_one(P.y, G.y, M.y, V.y, lr, beta1, beta2, eps, wd, bc1, bc2s);
    adamw_one(P.z, G.z, M.z, V.z, lr, beta1, beta2, eps, wd, bc1, bc2s);
    adamw_one(P.w, G.w, M.w, V.w, lr, beta1, beta2, eps, wd, bc1, bc2s);
    p4[i] = P;
    m4[i] = M;
    v4[i] = V;
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {  // up to 3 head + 3 tail elements
    const int tail = (int)(n - head - n4 * 4);
    long long i = -1;
    if ((int)threadIdx.x < head) i = threadIdx.x;
    else if ((int)threadIdx.x >= 4 && (int)threadIdx.x - 4 < tail) i = head + n4 * 4 + (threadIdx.x - 4);
    if (i >= 0) {
      float P = p[i], M = m[i], V = v[i];
      adamw_one(P, g[i], M, V, lr, beta1, beta2, eps, wd, bc1, bc2s);
      p[i] = P; m[i] = M; v[i] = V;
    }
  }
}

int loss_blocks(long long n) {
  long long b = (n + LT - 1) / LT;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }

struct LossLayout {         // partials at 0; masked: the count pairs and {N, N_g} between them and the sign bytes
  int blocks = 0;
  size_t cnt = 0, nn = 0, sg = 0, bytes = 0;
};

LossLayout layout(long long n, bool masked) {
  LossLayout L;
  L.blocks = loss_blocks(n);
  size_t off = al16((size_t)L.blocks * 3 * sizeof(float));
  if (masked) {
    L.cnt = off; off += al16((size_t)L.blocks * 2 * sizeof(unsigned int));
    L.nn = off; off += 16;
  }
  L.sg = off;
  L.bytes = off + (size_t)n * 2;
  return L;
}

// valid NULL is an error of a masked entry; an unmasked one passes NULL and masked = false
int loss_forward(bool masked, const float* pred, const float* gt, const unsigned char* valid, float w1, float w2, float wg,
                 float* losses, void* workspace, int B, int H, int W, jspsr_stream_t stream) {
  const char* name = masked ? "loss_valid_forward" : "loss_forward";
  if (!pred || !gt || (masked && !valid) || !losses || !workspace || B <= 0 || H <= 0 || W <= 0)
    return fail(JSPSR_EINVAL, "%s: bad arguments", name);
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "%s: workspace not 16-byte aligned", name);
  const long long n = (long long)B * H * W;
  const LossLayout L = layout(n, masked);
  char* ws = static_cast<char*>(workspace);
  float* partial = reinterpret_cast<float*>(ws);
  unsigned int* pcnt = reinterpret_cast<unsigned int*>(ws + L.cnt);
  signed char* sg = reinterpret_cast<signed char*>(ws + L.sg);
  long long* nn = reinterpret_cast<long long*>(ws + L.nn);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (masked) {
    hipLaunchKernelGGL(loss_fwd_kernel<true>, dim3(L.blocks), dim3(LT), 0, s, pred, gt, valid, sg, partial, pcnt, B, H, W);
    if (int e = check_launch("loss_valid_forward")) return e;
    hipLaunchKernelGGL(loss_finalize_kernel<true>, dim3(1), dim3(320), 0, s, partial, pcnt, L.blocks, n, w1, w2, wg, losses, nn);
    return check_launch("loss_valid_finalize");
  }
  hipLaunchKernelGGL(loss_fwd_kernel<false>, dim3(L.blocks), dim3(LT), 0, s, pred, gt, nullptr, sg, partial, nullptr, B, H, W);
  if (int e = check_launch("loss_forward")) return e;
  hipLaunchKernelGGL(loss_finalize_kernel<false>, dim3(1), dim3(192), 0, s, partial, nullptr, L.blocks, n, w1, w2, wg, losses,
                     nullptr);
  return check_launch("loss_finalize");
}

int loss_backward(bool masked, const float* pred, const float* gt, const unsigned char* valid, const float* grad_total,
                  float w1, float w2, float wg, float* grad_pred, const void* workspace, int B, int H, int W,
                  jspsr_stream_t stream) {
  const char* name = masked ? "loss_valid_backward" : "loss_backward";
  if (!pred || !gt || (masked && !valid) || !grad_pred || !workspace || B <= 0 || H <= 0 || W <= 0)
    return fail(JSPSR_EINVAL, "%s: bad arguments", name);
  if (!aligned16(workspace)) return fail(JSPSR_EALIGN, "%s: workspace not 16-byte aligned", name);
  const LossLayout L = layout((long long)B * H * W, masked);
  const char* ws = static_cast<const char*>(workspace);
  const signed char* sg = reinterpret_cast<const signed char*>(ws + L.sg);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (masked) {
    hipLaunchKernelGGL(loss_bwd_kernel<true>, dim3(L.blocks), dim3(LT), 0, s, pred, gt, valid, sg,
                       reinterpret_cast<const long long*>(ws + L.nn), grad_total, w1, w2, wg, grad_pred, B, H, W);
    return check_launch("loss_valid_backward");
  }
  hipLaunchKernelGGL(loss_bwd_kernel<false>, dim3(L.blocks), dim3(LT), 0, s, pred, gt, nullptr, sg, nullptr, grad_total, w1, w2,
                     wg, grad_pred, B, H, W);
  return check_launch("loss_backward");
}

}  // namespace

extern "C" size_t jspsr_loss_workspace_bytes(int B, int H, int W) {
  return B <= 0 || H <= 0 || W <= 0 ? 0 : layout((long long)B * H * W, false).bytes;
}

extern "C" size_t jspsr_loss_valid_workspace_bytes(int B, int H, int W) {
  return B <= 0 || H <= 0 || W <= 0 ? 0 : layout((long long)B * H * W, true).bytes;
}

extern "C" int jspsr_loss_forward(const float* pred, const float* gt, float w1, float w2, float wg, float* losses,
                                  void* workspace, int B, int H, int W, jspsr_stream_t stream) {
  return loss_forward(false, pred, gt, nullptr, w1, w2, wg, losses, workspace, B, H, W, stream);
}

extern "C" int jspsr_loss_backward(const float* pred, const float* gt, const float* grad_total, float w1, float w2,
                                   float wg, float* grad_pred, const void* workspace, int B, int H, int W,
                                   jspsr_stream_t stream) {
  return loss_backward(false, pred, gt, nullptr, grad_total, w1, w2, wg, grad_pred, workspace, B, H, W, stream);
}

extern "C" int jspsr_loss_valid_forward(const float* pred, const float* gt, const unsigned char* valid, float w1, float w2,
                                        float wg, float* losses, void* workspace, int B, int H, int W, jspsr_stream_t stream) {
  return loss_forward(true, pred, gt, valid, w1, w2, wg, losses, workspace, B, H, W, stream);
}

extern "C" int jspsr_loss_valid_backward(const float* pred, const float* gt, const unsigned char* valid,
                                         const float* grad_total, float w1, float w2, float wg, float* grad_pred,
                                         const void* workspace, int B, int H, int W, jspsr_stream_t stream) {
  return loss_backward(true, pred, gt, valid, grad_total, w1, w2, wg, grad_pred, workspace, B, H, W, stream);
}

extern "C" int jspsr_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                                float beta1, float beta2, float eps, float weight_decay, int step, jspsr_stream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return fail(JSPSR_EINVAL, "adamw_step: bad arguments");
  const uintptr_t mis = reinterpret_cast<uintptr_t>(param) & 15;
  if ((mis & 3) || (reinterpret_cast<uintptr_t>(grad) & 15) != mis || (reinterpret_cast<uintptr_t>(exp_avg) & 15) != mis ||
      (reinterpret_cast<uintptr_t>(exp_avg_sq) & 15) != mis)
    return fail(JSPSR_EALIGN, "adamw_step: buffers must be 4-byte aligned and equally offset from a 16-byte boundary");
  int head = (int)(((16 - mis) & 15) >> 2);
  if (head > n) head = (int)n;
  // bias corrections in double on the host, as torch.optim.AdamW computes them (float powf is ~3e-5 relative off at
  // small step counts)
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  long long b = (n / 4 + 255) / 256;
  const int blocks = (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), param, grad, exp_avg,
                     exp_avg_sq, n, head, lr, beta1, beta2, eps, weight_decay, bc1, bc2s);
  return check_launch("adamw_step");
}

extern "C" int jspsr_adamw_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                                    const float* hyper, jspsr_stream_t stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !hyper || n <= 0) return fail(JSPSR_EINVAL, "adamw_step_dev: bad arguments");
  const uintptr_t mis = reinterpret_cast<uintptr_t>(param) & 15;
  if ((mis & 3) || (reinterpret_cast<uintptr_t>(grad) & 15) != mis || (reinterpret_cast<uintptr_t>(exp_avg) & 15) != mis ||
      (reinterpret_cast<uintptr_t>(exp_avg_sq) & 15) != mis || (reinterpret_cast<uintptr_t>(hyper) & 3))
    return fail(JSPSR_EALIGN, "adamw_step_dev: buffers must be 4-byte aligned and equally offset from a 16-byte boundary");
  int head = (int)(((16 - mis) & 15) >> 2);
  if (head > n) head = (int)n;
  long long b = (n / 4 + 255) / 256;
  const int blocks = (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
  hipLaunchKernelGGL(adamw_dev_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), param, grad, exp_avg,
                     exp_avg_sq, n, head, hyper);
  return check_launch("adamw_step");
}
