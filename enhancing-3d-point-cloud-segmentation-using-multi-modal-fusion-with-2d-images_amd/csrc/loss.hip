// Segmentation loss of KPFCNN in three launches, forward and backward together (reference: KPConv-PyTorch/models/architectures.py:345-372 --
// labels outside `valid_labels` become -1, then torch.nn.CrossEntropyLoss(weight=class_w, ignore_index=-1) on the
// logits transposed to (1, C, N); mean over the kept points weighted by the class weights):
//     loss = sum_i w[t_i] * (logsumexp(x_i) - x_i[t_i]) / sum_i w[t_i]            (i over points with t_i >= 0)
//     dx_i = g * w[t_i] / sum_j w[t_j] * (softmax(x_i) - onehot(t_i))             (0 for ignored points)
// As library calls the same is ~12 launches at the turn-around of every step (label lookup x3, transpose copy, 2-D
// log-softmax, nll_loss2d + its size-average kernel, and their backward kernels with a zero fill).
// Forward: one thread per point, workgroup partial sums, then one small workgroup adds the partials in order
// (deterministic; a kernel boundary instead of an in-kernel agent-scope fence, which on the 8 XCDs means L2
// write-backs under the other branches of the step). Backward recomputes the softmax (C is ~20).
// The second half of this file is the MVPNet baseline's loss and metrics on channel-first logits (seg_*), which shares
// the ordered finish.
#include "common.h"

namespace {

constexpr int XT = 256;        // points per workgroup
constexpr int XC_MAX = 256;    // classes

template <bool L64>
__device__ __forceinline__ int class_of(const void* labels, int64_t i, const int32_t* __restrict__ lut, int lut_n) {
  // architectures.py:352-355: any value that is not a valid label -> -1 (lut[0] serves negatives, lut[lut_n-1] the
  // values above the table)
  int64_t l = L64 ? ((const int64_t*)labels)[i] : (int64_t)((const int32_t*)labels)[i];
  l = l < -1 ? -1 : (l > lut_n - 2 ? lut_n - 2 : l);
  return lut[l + 1];
}

template <bool L64>
__global__ __launch_bounds__(XT) void xent_fwd_k(const float* __restrict__ x, int64_t N, int C, const void* labels,
                                                 const int32_t* __restrict__ lut, int lut_n,
                                                 const float* __restrict__ weight, float* __restrict__ partials) {
  __shared__ float sl[XT / 64], sw[XT / 64];
  const int64_t i = (int64_t)blockIdx.x * XT + threadIdx.x;
  float li = 0.f, wi = 0.f;
  if (i < N) {
    const int t = class_of<L64>(labels, i, lut, lut_n);
    if (t >= 0 && t < C) {
      const float* r = x + i * C;
      float m = r[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, r[c]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) s += expf(r[c] - m);
      wi = weight ? weight[t] : 1.f;
      li = wi * (logf(s) + m - r[t]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    li += __shfl_xor(li, o);
    wi += __shfl_xor(wi, o);
  }
  if ((threadIdx.x & 63) == 0) {
    sl[threadIdx.x >> 6] = li;
    sw[threadIdx.x >> 6] = wi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < XT / 64; ++w) {
      a += sl[w];
      b += sw[w];
    }
    partials[2 * blockIdx.x] = a;
    partials[2 * blockIdx.x + 1] = b;
  }
}

// one wave: lane l adds partials l, l + 64, ... in order, then the 64 lane sums are added in lane order
template <typename T = float>
__global__ __launch_bounds__(64) void xent_finish_k(const T* __restrict__ partials, int nblk, T* __restrict__ out2) {
  __shared__ T sa[64], sb[64];
  T a = 0, b = 0;
  for (int g = threadIdx.x; g < nblk; g += 64) {
    a += partials[2 * g];
    b += partials[2 * g + 1];
  }
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0;
    b = 0;
    for (int l = 0; l < 64; ++l) {
      a += sa[l];
      b += sb[l];
    }
    out2[0] = a / b;                     // no kept point: 0 / 0 = NaN, like torch's mean over an empty set
    out2[1] = b;
  }
}

template <bool L64>
__global__ __launch_bounds__(XT) void xent_bwd_k(const float* __restrict__ x, int64_t N, int C, const void* labels,
                                                 const int32_t* __restrict__ lut, int lut_n,
                                                 const float* __restrict__ weight, const float* __restrict__ out2,
                                                 const float* __restrict__ g, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * XT + threadIdx.x;
  if (i >= N) return;
  const int t = class_of<L64>(labels, i, lut, lut_n);
  float* d = dx + i * C;
  if (t < 0 || t >= C) {
    for (int c = 0; c < C; ++c) d[c] = 0.f;
    return;
  }
  const float* r = x + i * C;
  float m = r[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, r[c]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(r[c] - m);
  const float k = g[0] * (weight ? weight[t] : 1.f) / out2[1], inv = 1.f / s;
  for (int c = 0; c < C; ++c) d[c] = k * (expf(r[c] - m) * inv - (c == t ? 1.f : 0.f));
}

}  // namespace

extern "C" int64_t mvk_xent_workspace_floats(int64_t N) { return 2 * cdiv64(N > 0 ? N : 1, XT); }

extern "C" int mvk_xent_fwd(const float* logits, int64_t N, int C, const void* labels, int labels64,
                            const int32_t* lut, int lut_n, const float* class_weight, float* partials, float* out2,
                            void* stream) {
  MVK_REQUIRE(N >= 0 && C > 0 && C <= XC_MAX && lut_n >= 3, "xent: bad sizes N=%lld C=%d lut=%d", (long long)N, C, lut_n);
  MVK_REQUIRE(lut && partials && out2 && (N == 0 || (logits && labels)), "xent: null operand");
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)cdiv64(N > 0 ? N : 1, XT);
  if (labels64)
    hipLaunchKernelGGL(xent_fwd_k<true>, dim3(gx), dim3(XT), 0, st, logits, N, C, labels, lut, lut_n, class_weight, partials);
  else
    hipLaunchKernelGGL(xent_fwd_k<false>, dim3(gx), dim3(XT), 0, st, logits, N, C, labels, lut, lut_n, class_weight, partials);
  hipLaunchKernelGGL(xent_finish_k<float>, dim3(1), dim3(64), 0, st, partials, (int)gx, out2);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_xent_bwd(const float* logits, int64_t N, int C, const void* labels, int labels64, const int32_t* lut,
                            int lut_n, const float* class_weight, const float* out2, const float* grad_loss,
                            float* dlogits, void* stream) {
  MVK_REQUIRE(N >= 0 && C > 0 && C <= XC_MAX && lut_n >= 3, "xent: bad sizes");
  if (N == 0) return 0;
  MVK_REQUIRE(logits && labels && lut && out2 && grad_loss && dlogits, "xent: null operand");
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)cdiv64(N, XT);
  if (labels64)
    hipLaunchKernelGGL(xent_bwd_k<true>, dim3(gx), dim3(XT), 0, st, logits, N, C, labels, lut, lut_n, class_weight, out2,
                       grad_loss, dlogits);
  else
    hipLaunchKernelGGL(xent_bwd_k<false>, dim3(gx), dim3(XT), 0, st, logits, N, C, labels, lut, lut_n, class_weight, out2,
                       grad_loss, dlogits);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Segmentation loss and metrics of the MVPNet baseline (reference mvpnet/models/loss.py, metric.py) on CHANNEL-FIRST
// logits (B, C, S), S the product of the trailing dimensions, labels (B, S): what F.cross_entropy(weight, ignore_index),
// two argmax(1), two mask indexings, a sum and a bincount compute, from one read of the logits.
//   kept(i)  : label != ignore_index and 0 <= label < C. ignore_index wins even when it is itself a class number. A label
//              that is neither sets *status = 1 and is otherwise treated like an ignored one (nothing faults).
//   lse_i    = log sum_c exp(x[b, c, s])                                     (stored for the backward, one T per point)
//   loss     = sum_kept w[t_i] (lse_i - x[b, t_i, s]) / sum_kept w[t_i]      (0 / 0 = NaN with no kept point, like torch)
//   pred_i   = the LOWEST class index among the maximal logits (what torch.argmax documents)
//   counts   = (#kept with pred == label, #kept);  conf[label * C + pred] += 1 over the kept points
//   dx[b,c,s]= g w[t_i] / sum_kept w * (exp(x[b,c,s] - lse_i) - [c == t_i]),  0 for every class of a point not kept
// A NaN logit is outside the contract (pred and loss are then unspecified; nothing faults). A logit of -inf is a class
// of probability 0, as in torch.
// One lane per point: for every class a wave reads 64 consecutive elements (a wave may straddle a batch boundary, so
// b and s are per lane). One pass with a running maximum and a rescaled sum: every logit is loaded once and costs one
// exp. Loss and weight: wave shuffles, LDS, one partial pair per workgroup, xent_finish_k adds them in fixed order (no
// float atomics: bit-equal from run to run). The counts are integers, so their atomics are exact in any arrival order:
// hits / kept by wave ballots and one 64-bit add per workgroup, the confusion in an int32 LDS histogram (C <= 64,
// 16 KiB) flushed with one 64-bit add per non-zero bin, above that one global add per kept point.
namespace {

constexpr int SEG_LDS_C = 64;                          // largest C whose confusion fits the LDS histogram
enum { SEG_CONF_NONE = 0, SEG_CONF_LDS = 1, SEG_CONF_GLOBAL = 2 };

__device__ __forceinline__ float seg_exp(float v) { return expf(v); }
__device__ __forceinline__ double seg_exp(double v) { return exp(v); }
__device__ __forceinline__ float seg_log(float v) { return logf(v); }
__device__ __forceinline__ double seg_log(double v) { return log(v); }

template <bool L64>
__device__ __forceinline__ int seg_class(const void* labels, int64_t i, int64_t ignore, int C, int32_t* status) {
  const int64_t l = L64 ? ((const int64_t*)labels)[i] : (int64_t)((const int32_t*)labels)[i];
  if (l == ignore) return -1;
  if (l < 0 || l >= C) {
    if (status) *status = 1;
    return -1;
  }
  return (int)l;
}

// LOSS false: predictions only (no exp, no lse, no partials)
template <typename T, bool L64, bool LOSS, int CM>
__global__ __launch_bounds__(XT) void seg_fwd_k(const T* __restrict__ x, int64_t P, int C, int64_t S, const void* labels,
                                                int64_t ignore, const T* __restrict__ weight, T* __restrict__ partials,
                                                T* __restrict__ lse, unsigned long long* counts, unsigned long long* conf,
                                                int32_t* status) {
  __shared__ T sl[XT / 64], sw[XT / 64];
  __shared__ int sh[XT / 64], sk[XT / 64];
  __shared__ int hist[CM == SEG_CONF_LDS ? SEG_LDS_C * SEG_LDS_C : 1];
  if (CM == SEG_CONF_LDS) {
    for (int b = threadIdx.x; b < C * C; b += XT) hist[b] = 0;
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * XT + threadIdx.x;
  T li = 0, wi = 0;
  bool kept = false, hit = false;
  if (i < P) {
    const int t = seg_class<L64>(labels, i, ignore, C, status);
    if (t >= 0) {
      kept = true;
      const int64_t b = i / S;
      const T* r = x + (b * C * S + (i - b * S));
      T m = r[0], s = 1, xt = m;
      int pred = 0;
#pragma unroll 4
      for (int c = 1; c < C; ++c) {
        const T v = r[c * S];
        const bool up = v > m;                         // strict: the first of equal maxima stays
        if (LOSS) {
          if (c == t) xt = v;
          const T e = seg_exp(up ? m - v : v - m);
          s = up ? s * e + 1 : (v == -INFINITY ? s : s + e);      // (-inf) - (-inf) would be NaN
        }
        if (up) {
          m = v;
          pred = c;
        }
      }
      hit = pred == t;
      if (LOSS) {
        const T l = m + seg_log(s);
        if (lse) lse[i] = l;
        wi = weight ? weight[t] : (T)1;
        li = wi * (l - xt);
      }
      if (CM == SEG_CONF_LDS) atomicAdd(&hist[t * C + pred], 1);
      if (CM == SEG_CONF_GLOBAL) atomicAdd(conf + (t * C + pred), 1ull);
    }
  }
  if (LOSS) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      li += __shfl_xor(li, o);
      wi += __shfl_xor(wi, o);
    }
  }
  const unsigned long long km = __ballot(kept), hm = __ballot(hit);
  if ((threadIdx.x & 63) == 0) {
    if (LOSS) {
      sl[threadIdx.x >> 6] = li;
      sw[threadIdx.x >> 6] = wi;
    }
    sk[threadIdx.x >> 6] = __popcll(km);
    sh[threadIdx.x >> 6] = __popcll(hm);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    T a = 0, b = 0;
    int k = 0, h = 0;
    for (int w = 0; w < XT / 64; ++w) {
      if (LOSS) {
        a += sl[w];
        b += sw[w];
      }
      k += sk[w];
      h += sh[w];
    }
    if (LOSS) {
      partials[2 * blockIdx.x] = a;
      partials[2 * blockIdx.x + 1] = b;
    }
    if (counts) {
      if (h) atomicAdd(counts, (unsigned long long)h);
      if (k) atomicAdd(counts + 1, (unsigned long long)k);
    }
  }
  if (CM == SEG_CONF_LDS) {                            // every LDS add above is before the barrier
    for (int b = threadIdx.x; b < C * C; b += XT) {
      const int v = hist[b];
      if (v) atomicAdd(conf + b, (unsigned long long)v);
    }
  }
}

template <typename T, bool L64>
__global__ __launch_bounds__(XT) void seg_bwd_k(const T* __restrict__ x, int64_t P, int C, int64_t S, const void* labels,
                                                int64_t ignore, const T* __restrict__ weight, const T* __restrict__ out2,
                                                const T* __restrict__ lse, const T* __restrict__ g, T* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * XT + threadIdx.x;
  if (i >= P) return;
  const int t = seg_class<L64>(labels, i, ignore, C, nullptr);
  const int64_t b = i / S, off = b * C * S + (i - b * S);
  T* d = dx + off;
  if (t < 0) {
    for (int c = 0; c < C; ++c) d[c * S] = 0;
    return;
  }
  const T* r = x + off;
  const T k = g[0] * (weight ? weight[t] : (T)1) / out2[1], l = lse[i];
#pragma unroll 4
  for (int c = 0; c < C; ++c) d[c * S] = k * (seg_exp(r[c * S] - l) - (c == t ? (T)1 : (T)0));
}

template <typename T, bool L64, bool LOSS>
void seg_fwd_pick(int cm, unsigned gx, hipStream_t st, const T* x, int64_t P, int C, int64_t S, const void* labels,
                  int64_t ignore, const T* weight, T* partials, T* lse, unsigned long long* counts,
                  unsigned long long* conf, int32_t* status) {
  if (cm == SEG_CONF_LDS)
    hipLaunchKernelGGL((seg_fwd_k<T, L64, LOSS, SEG_CONF_LDS>), dim3(gx), dim3(XT), 0, st, x, P, C, S, labels, ignore, weight,
                       partials, lse, counts, conf, status);
  else if (cm == SEG_CONF_GLOBAL)
    hipLaunchKernelGGL((seg_fwd_k<T, L64, LOSS, SEG_CONF_GLOBAL>), dim3(gx), dim3(XT), 0, st, x, P, C, S, labels, ignore,
                       weight, partials, lse, counts, conf, status);
  else
    hipLaunchKernelGGL((seg_fwd_k<T, L64, LOSS, SEG_CONF_NONE>), dim3(gx), dim3(XT), 0, st, x, P, C, S, labels, ignore, weight,
                       partials, lse, counts, conf, status);
}

template <typename T>
int seg_fwd(const T* logits, int64_t B, int C, int64_t S, const void* labels, int labels64, int64_t ignore, const T* weight,
            T* partials, T* out2, T* lse, int64_t* counts, int64_t* conf, int32_t* status, void* stream) {
  MVK_REQUIRE(B >= 0 && S >= 0 && C > 0 && C <= XC_MAX, "seg_loss: bad sizes B=%lld C=%d S=%lld", (long long)B, C, (long long)S);
  MVK_REQUIRE(S == 0 || B <= INT64_MAX / S / C, "seg_loss: B * C * S overflows");
  const int64_t P = B * S;
  const bool loss = out2 != nullptr;
  MVK_REQUIRE(loss ? partials != nullptr : (!partials && !lse && (counts || conf)),
              "seg_loss: the loss form needs partials and out2, the metrics-only form neither nor lse, and counts or conf");
  MVK_REQUIRE(P == 0 || (logits && labels), "seg_loss: null operand");
  const int64_t gx = cdiv64(P > 0 ? P : 1, XT);
  MVK_REQUIRE(gx <= 0x7fffffffLL, "seg_loss: too many points");
  if (!loss && P == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int cm = !conf ? SEG_CONF_NONE : (C <= SEG_LDS_C ? SEG_CONF_LDS : SEG_CONF_GLOBAL);
  unsigned long long *cn = (unsigned long long*)counts, *cf = (unsigned long long*)conf;
  if (loss) {
    if (labels64)
      seg_fwd_pick<T, true, true>(cm, (unsigned)gx, st, logits, P, C, S, labels, ignore, weight, partials, lse, cn, cf, status);
    else
      seg_fwd_pick<T, false, true>(cm, (unsigned)gx, st, logits, P, C, S, labels, ignore, weight, partials, lse, cn, cf, status);
    hipLaunchKernelGGL(xent_finish_k<T>, dim3(1), dim3(64), 0, st, partials, (int)gx, out2);
  } else {
    if (labels64)
      seg_fwd_pick<T, true, false>(cm, (unsigned)gx, st, logits, P, C, S, labels, ignore, nullptr, nullptr, nullptr, cn, cf, status);
    else
      seg_fwd_pick<T, false, false>(cm, (unsigned)gx, st, logits, P, C, S, labels, ignore, nullptr, nullptr, nullptr, cn, cf, status);
  }
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int seg_bwd(const T* logits, int64_t B, int C, int64_t S, const void* labels, int labels64, int64_t ignore, const T* weight,
            const T* out2, const T* lse, const T* grad_loss, T* dlogits, void* stream) {
  MVK_REQUIRE(B >= 0 && S >= 0 && C > 0 && C <= XC_MAX, "seg_loss: bad sizes B=%lld C=%d S=%lld", (long long)B, C, (long long)S);
  MVK_REQUIRE(S == 0 || B <= INT64_MAX / S / C, "seg_loss: B * C * S overflows");
  const int64_t P = B * S;
  if (P == 0) return 0;
  MVK_REQUIRE(logits && labels && out2 && lse && grad_loss && dlogits, "seg_loss: null operand");
  const int64_t gx = cdiv64(P, XT);
  MVK_REQUIRE(gx <= 0x7fffffffLL, "seg_loss: too many points");
  hipStream_t st = (hipStream_t)stream;
  if (labels64)
    hipLaunchKernelGGL((seg_bwd_k<T, true>), dim3((unsigned)gx), dim3(XT), 0, st, logits, P, C, S, labels, ignore, weight, out2,
                       lse, grad_loss, dlogits);
  else
    hipLaunchKernelGGL((seg_bwd_k<T, false>), dim3((unsigned)gx), dim3(XT), 0, st, logits, P, C, S, labels, ignore, weight, out2,
                       lse, grad_loss, dlogits);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int64_t mvk_seg_workspace_floats(int64_t points) { return 2 * cdiv64(points > 0 ? points : 1, XT); }

extern "C" int mvk_seg_loss_fwd(const float* logits, int64_t B, int C, int64_t S, const void* labels, int labels64,
                                int64_t ignore_index, const float* class_weight, float* partials, float* out2, float* lse,
                                int64_t* counts, int64_t* conf, int32_t* status, void* stream) {
  return seg_fwd<float>(logits, B, C, S, labels, labels64, ignore_index, class_weight, partials, out2, lse, counts, conf, status,
                        stream);
}

extern "C" int mvk_seg_loss_fwd_f64(const double* logits, int64_t B, int C, int64_t S, const void* labels, int labels64,
                                    int64_t ignore_index, const double* class_weight, double* partials, double* out2,
                                    double* lse, int64_t* counts, int64_t* conf, int32_t* status, void* stream) {
  return seg_fwd<double>(logits, B, C, S, labels, labels64, ignore_index, class_weight, partials, out2, lse, counts, conf,
                         status, stream);
}

extern "C" int mvk_seg_loss_bwd(const float* logits, int64_t B, int C, int64_t S, const void* labels, int labels64,
                                int64_t ignore_index, const float* class_weight, const float* out2, const float* lse,
                                const float* grad_loss, float* dlogits, void* stream) {
  return seg_bwd<float>(logits, B, C, S, labels, labels64, ignore_index, class_weight, out2, lse, grad_loss, dlogits, stream);
}

extern "C" int mvk_seg_loss_bwd_f64(const double* logits, int64_t B, int C, int64_t S, const void* labels, int labels64,
                                    int64_t ignore_index, const double* class_weight, const double* out2, const double* lse,
                                    const double* grad_loss, double* dlogits, void* stream) {
  return seg_bwd<double>(logits, B, C, S, labels, labels64, ignore_index, class_weight, out2, lse, grad_loss, dlogits, stream);
}
