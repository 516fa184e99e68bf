// K11: the reference's optimizer menu over ONE flat parameter / gradient buffer (utils/common_config.py:241-291 builds
// torch.optim.SGD / Adam / AdamW / RMSprop), with the gradient range of the training monitor fused into the step
// (train/train_utils.py:127-143, get_gradient_range: ~900 per-tensor min / max launches there, no extra HBM traffic here),
// and the min / max of a few whole tensors for `monitor_value: input / pred` (get_tensor_range, :84-96).
//
// One kernel template for the four updates: a scalar head brings the (equally misaligned) buffers to a 16-byte boundary,
// then float4s, then a tail -- the shape of adamw_kernel in train_step.hip, which stays the step of a FlatAdamW that
// monitors nothing.  All of it is HBM-bound: 12 B (SGD) to 28 B (Adam, RMSprop with momentum) per parameter.
#include <cfloat>
#include <cmath>

#include "common.h"

namespace {

using namespace jspsr;

constexpr int OT = 256;            // threads per workgroup
constexpr int MAX_BLOCKS = 4096;   // rows of the range workspace
constexpr int TR_BLOCKS = 64;      // workgroups per tensor of jspsr_tensor_ranges
constexpr int TR_MAX = 8;

// lr, a, b, eps, weight decay, c1, c2: the row jspsr_optim_step documents (include/jspsr_hip.h)
struct Hyper {
  float lr, a, b, eps, wd, c1, c2;
};

// min / max over the FINITE values seen, and how many were not finite
struct Range {
  float mn = INFINITY, mx = -INFINITY, bad = 0.f;
  __device__ __forceinline__ void add(float x) {
    if (fabsf(x) <= FLT_MAX) {
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    } else {
      bad += 1.f;
    }
  }
  __device__ __forceinline__ void merge(float omn, float omx, float obad) {
    mn = fminf(mn, omn);
    mx = fmaxf(mx, omx);
    bad += obad;
  }
};

// wave reduction, then one value per wave through LDS: afterwards thread 0 holds the workgroup's range
__device__ __forceinline__ void block_reduce(Range& r) {
  __shared__ float red[3][OT / 64];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) r.merge(__shfl_xor(r.mn, d, 64), __shfl_xor(r.mx, d, 64), __shfl_xor(r.bad, d, 64));
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = r.mn;
    red[1][threadIdx.x >> 6] = r.mx;
    red[2][threadIdx.x >> 6] = r.bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    r = Range();
    for (int w = 0; w < OT / 64; ++w) r.merge(red[0][w], red[1][w], red[2][w]);
  }
}

// One element of each update, torch's semantics at its defaults (maximize=False, foreach / fused irrelevant).
//   SGD      S1 = momentum_buffer (MOM only).  h.a momentum, h.c1 != 0: the first step, where the buffer IS the gradient.
//   Adam     S1 = exp_avg, S2 = exp_avg_sq; coupled L2.  h.a beta1, h.b beta2, h.c1 = 1 - beta1^t, h.c2 = sqrt(1 - beta2^t).
//   AdamW    the same with decoupled decay: adamw_one of train_step.hip, expression for expression.
//   RMSprop  S1 = square_avg, S2 = momentum_buffer (MOM only); eps OUTSIDE the root, not centered.  h.a momentum, h.b alpha.
template <int K, bool MOM>
__device__ __forceinline__ void update_one(float& P, float G, float& S1, float& S2, const Hyper& h) {
  if constexpr (K == JSPSR_OPT_ADAMW) {
    P *= 1.f - h.lr * h.wd;
  } else {
    G += h.wd * P;
  }
  if constexpr (K == JSPSR_OPT_SGD) {
    if constexpr (MOM) {
      S1 = h.c1 != 0.f ? G : h.a * S1 + G;
      G = S1;
    }
    P -= h.lr * G;
  } else if constexpr (K == JSPSR_OPT_RMSPROP) {
    S1 = h.b * S1 + (1.f - h.b) * G * G;
    const float q = G / (sqrtf(S1) + h.eps);
    if constexpr (MOM) {
      S2 = h.a * S2 + q;
      P -= h.lr * S2;
    } else {
      P -= h.lr * q;
    }
  } else {
    S1 = h.a * S1 + (1.f - h.a) * G;
    S2 = h.b * S2 + (1.f - h.b) * G * G;
    P -= (h.lr / h.c1) * S1 / (sqrtf(S2) / h.c2 + h.eps);
  }
}

// `hyper` non-null: the seven scalars come from DEVICE memory (a launch captured in a hipGraph carries its kernel
// arguments verbatim; the caller refreshes the row before every replay).  Same arithmetic, same bits.
// RANGE: the workgroup's range of the gradient it has just read goes to partial[blockIdx.x][0..2].
template <int K, bool MOM, bool RANGE>
__global__ __launch_bounds__(OT) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                  float* __restrict__ s2, long long n, int head, Hyper h,
                                                  const float* __restrict__ hyper, float* __restrict__ partial) {
  constexpr bool U1 = K != JSPSR_OPT_SGD || MOM;                                             // is S1 / S2 state of this update?
  constexpr bool U2 = K == JSPSR_OPT_ADAM || K == JSPSR_OPT_ADAMW || (K == JSPSR_OPT_RMSPROP && MOM);
  if (hyper) h = Hyper{hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5], hyper[6]};
  const long long n4 = (n - head) / 4;
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* a4 = reinterpret_cast<float4*>(s1 + head);
  float4* b4 = reinterpret_cast<float4*>(s2 + head);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  Range r;
  for (long long i = blockIdx.x * (long long)OT + threadIdx.x; i < n4; i += (long long)gridDim.x * OT) {
    float4 P = p4[i];
    const float4 G = g4[i];
    float4 A = zero, B = zero;
    if constexpr (U1) A = a4[i];
    if constexpr (U2) B = b4[i];
    if constexpr (RANGE) {
      r.add(G.x); r.add(G.y); r.add(G.z); r.add(G.w);
    }
    update_one<K, MOM>(P.x, G.x, A.x, B.x, h);
    update_one<K, MOM>(P.y, G.y, A.y, B.y, h);
    update_one<K, MOM>(P.z, G.z, A.z, B.z, h);
    update_one<K, MOM>(P.w, G.w, A.w, B.w, h);
    p4[i] = P;
    if constexpr (U1) a4[i] = A;
    if constexpr (U2) b4[i] = B;
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) {  // up to 3 head + 3 tail elements
    const int tail = (int)(n - head - n4 * 4);
    long long i = -1;
    if ((int)threadIdx.x < head) i = threadIdx.x;
    else if ((int)threadIdx.x >= 4 && (int)threadIdx.x - 4 < tail) i = head + n4 * 4 + (threadIdx.x - 4);
    if (i >= 0) {
      float P = p[i], A = 0.f, B = 0.f;
      if constexpr (U1) A = s1[i];
      if constexpr (U2) B = s2[i];
      const float G = g[i];
      if constexpr (RANGE) r.add(G);
      update_one<K, MOM>(P, G, A, B, h);
      p[i] = P;
      if constexpr (U1) s1[i] = A;
      if constexpr (U2) s2[i] = B;
    }
  }
  if constexpr (RANGE) {
    block_reduce(r);
    if (threadIdx.x == 0) {
      partial[(size_t)blockIdx.x * 4 + 0] = r.mn;
      partial[(size_t)blockIdx.x * 4 + 1] = r.mx;
      partial[(size_t)blockIdx.x * 4 + 2] = r.bad;
    }
  }
}

// The last, small reduction: `rows` partials of each of gridDim.x tables -> out[blockIdx.x][0..2].  combine != 0: fold into
// what `out` holds already (several ranges of one step, and the caller's start values 999 / -999).
__global__ __launch_bounds__(OT) void range_finalize_kernel(const float* __restrict__ partial, int rows, int combine,
                                                           float* __restrict__ out) {
  const float* part = partial + (size_t)blockIdx.x * rows * 4;
  Range r;
  for (int i = threadIdx.x; i < rows; i += OT) r.merge(part[(size_t)i * 4], part[(size_t)i * 4 + 1], part[(size_t)i * 4 + 2]);
  block_reduce(r);
  if (threadIdx.x == 0) {
    float* o = out + (size_t)blockIdx.x * 4;
    if (combine) r.merge(o[0], o[1], o[2]);
    o[0] = r.mn;
    o[1] = r.mx;
    o[2] = r.bad;
    if (!combine) o[3] = 0.f;
  }
}

struct TensorList {
  const void* ptr[TR_MAX];
  long long n[TR_MAX];
  int dtype[TR_MAX];
};

__global__ __launch_bounds__(OT) void tensor_ranges_kernel(TensorList t, float* __restrict__ partial) {
  const int k = blockIdx.y;
  const long long n = t.n[k];
  Range r;
  if (t.dtype[k] == JSPSR_BF16) {
    const unsigned short* x = static_cast<const unsigned short*>(t.ptr[k]);
    for (long long i = blockIdx.x * (long long)OT + threadIdx.x; i < n; i += (long long)gridDim.x * OT)
      r.add(__uint_as_float((unsigned)x[i] << 16));
  } else {
    const float* x = static_cast<const float*>(t.ptr[k]);
    for (long long i = blockIdx.x * (long long)OT + threadIdx.x; i < n; i += (long long)gridDim.x * OT) r.add(x[i]);
  }
  block_reduce(r);
  if (threadIdx.x == 0) {
    float* o = partial + ((size_t)k * gridDim.x + blockIdx.x) * 4;
    o[0] = r.mn;
    o[1] = r.mx;
    o[2] = r.bad;
  }
}

template <int K, bool MOM>
void launch(bool range, int blocks, hipStream_t s, float* p, const float* g, float* s1, float* s2, long long n, int head,
            const Hyper& h, const float* hyper, float* partial) {
  if (range)
    hipLaunchKernelGGL((optim_kernel<K, MOM, true>), dim3(blocks), dim3(OT), 0, s, p, g, s1, s2, n, head, h, hyper, partial);
  else
    hipLaunchKernelGGL((optim_kernel<K, MOM, false>), dim3(blocks), dim3(OT), 0, s, p, g, s1, s2, n, head, h, hyper, partial);
}

}  // namespace

extern "C" size_t jspsr_optim_workspace_bytes(void) { return (size_t)MAX_BLOCKS * 4 * sizeof(float); }

extern "C" int jspsr_optim_step(int kind, float* param, const float* grad, float* state1, float* state2, long long n, float lr,
                                float a, float b, float eps, float weight_decay, int step, const float* hyper,
                                float* grad_range, void* workspace, jspsr_stream_t stream) {
  if (kind < JSPSR_OPT_SGD || kind > JSPSR_OPT_RMSPROP) return fail(JSPSR_EINVAL, "optim_step: unknown kind %d", kind);
  if (!param || !grad || n <= 0 || (!hyper && step <= 0)) return fail(JSPSR_EINVAL, "optim_step: bad arguments");
  const bool adam = kind == JSPSR_OPT_ADAM || kind == JSPSR_OPT_ADAMW;
  // which state buffers the update owns: SGD a momentum buffer or nothing, RMSprop square_avg and maybe a momentum buffer
  const bool mom = kind == JSPSR_OPT_SGD ? state1 != nullptr : (kind == JSPSR_OPT_RMSPROP ? state2 != nullptr : true);
  if ((kind != JSPSR_OPT_SGD && !state1) || (adam && !state2) || (kind == JSPSR_OPT_SGD && state2))
    return fail(JSPSR_EINVAL, "optim_step: state buffers do not fit the update (kind %d)", kind);
  if (grad_range && !workspace) return fail(JSPSR_EINVAL, "optim_step: grad_range needs a workspace (jspsr_optim_workspace_bytes)");
  const uintptr_t mis = reinterpret_cast<uintptr_t>(param) & 15;
  if ((mis & 3) || (reinterpret_cast<uintptr_t>(grad) & 15) != mis || (state1 && (reinterpret_cast<uintptr_t>(state1) & 15) != mis) ||
      (state2 && (reinterpret_cast<uintptr_t>(state2) & 15) != mis) || !aligned4(hyper) || !aligned4(grad_range) ||
      !aligned4(workspace))
    return fail(JSPSR_EALIGN, "optim_step: buffers must be 4-byte aligned and equally offset from a 16-byte boundary");
  int head = (int)(((16 - mis) & 15) >> 2);
  if (head > n) head = (int)n;
  Hyper h{lr, a, b, eps, weight_decay, 0.f, 0.f};
  if (adam && !hyper) {  // bias corrections in double on the host, as torch computes them (and as jspsr_adamw_step does)
    h.c1 = (float)(1.0 - pow((double)a, (double)step));
    h.c2 = (float)sqrt(1.0 - pow((double)b, (double)step));
  } else if (kind == JSPSR_OPT_SGD) {
    h.c1 = step == 1 ? 1.f : 0.f;
  }
  long long nb = (n / 4 + OT - 1) / OT;
  const int blocks = (int)(nb < 1 ? 1 : (nb > MAX_BLOCKS ? MAX_BLOCKS : nb));
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  const bool range = grad_range != nullptr;
  switch (kind * 2 + (mom ? 1 : 0)) {
    case JSPSR_OPT_SGD * 2: launch<JSPSR_OPT_SGD, false>(range, blocks, s, param, grad, state1, state2, n, head, h, hyper, partial); break;
    case JSPSR_OPT_SGD * 2 + 1: launch<JSPSR_OPT_SGD, true>(range, blocks, s, param, grad, state1, state2, n, head, h, hyper, partial); break;
    case JSPSR_OPT_ADAM * 2 + 1: launch<JSPSR_OPT_ADAM, true>(range, blocks, s, param, grad, state1, state2, n, head, h, hyper, partial); break;
    case JSPSR_OPT_ADAMW * 2 + 1: launch<JSPSR_OPT_ADAMW, true>(range, blocks, s, param, grad, state1, state2, n, head, h, hyper, partial); break;
    case JSPSR_OPT_RMSPROP * 2: launch<JSPSR_OPT_RMSPROP, false>(range, blocks, s, param, grad, state1, state2, n, head, h, hyper, partial); break;
    default: launch<JSPSR_OPT_RMSPROP, true>(range, blocks, s, param, grad, state1, state2, n, head, h, hyper, partial); break;
  }
  if (int e = check_launch("optim_step")) return e;
  if (range) {
    hipLaunchKernelGGL(range_finalize_kernel, dim3(1), dim3(OT), 0, s, partial, blocks, 1, grad_range);
    return check_launch("optim_step (range)");
  }
  return JSPSR_OK;
}

extern "C" size_t jspsr_tensor_ranges_workspace_bytes(void) { return (size_t)TR_MAX * TR_BLOCKS * 4 * sizeof(float); }

extern "C" int jspsr_tensor_ranges(int count, const void* const* tensors, const long long* numel, const int* dtypes, float* table,
                                   void* workspace, jspsr_stream_t stream) {
  if (count < 1 || count > TR_MAX || !tensors || !numel || !dtypes || !table || !workspace)
    return fail(JSPSR_EINVAL, "tensor_ranges: 1..%d tensors, no null pointer", TR_MAX);
  TensorList t{};
  for (int k = 0; k < count; ++k) {
    if (!tensors[k] || numel[k] <= 0 || (dtypes[k] != JSPSR_F32 && dtypes[k] != JSPSR_BF16))
      return fail(JSPSR_EINVAL, "tensor_ranges: tensor %d is null, empty or neither fp32 nor bf16", k);
    if (reinterpret_cast<uintptr_t>(tensors[k]) & (dtypes[k] == JSPSR_F32 ? 3 : 1))
      return fail(JSPSR_EALIGN, "tensor_ranges: tensor %d is not aligned to its element size", k);
    t.ptr[k] = tensors[k];
    t.n[k] = numel[k];
    t.dtype[k] = dtypes[k];
  }
  if (!aligned4(table) || !aligned4(workspace)) return fail(JSPSR_EALIGN, "tensor_ranges: table / workspace must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(tensor_ranges_kernel, dim3(TR_BLOCKS, count), dim3(OT), 0, s, t, partial);
  if (int e = check_launch("tensor_ranges")) return e;
  hipLaunchKernelGGL(range_finalize_kernel, dim3(count), dim3(OT), 0, s, partial, TR_BLOCKS, 0, table);
  return check_launch("tensor_ranges (finalize)");
}
