// Test-time voting on the device (reference: KPConv-PyTorch/utils/tester.py:160-186, :223-236, :273-297 and
// utils/trainer.py:351-378, :395-412, :497-506) and the frozen BatchNorm apply of the inference forward.
//
// The reference copies every batch's probabilities to the host and runs a Python loop over spheres with NumPy fancy
// indexing into float64 per-cloud vote arrays; whole clouds later go through np.insert / argmax / confusion_matrix.
// Here the votes of all clouds live in one float64 buffer in HBM ([sum of cloud sizes, C], a row-offset table per
// cloud) and three kernels restate those lines:
//   vote_update_k    softmax in float32 (the reference rounds probabilities to float32 before they reach the float64
//                    accumulator), inner-sphere mask on (x*x + y*y) + z*z in float32, then
//                    votes[row] = smooth * votes[row] + one_minus_smooth * (double)p with two roundings (this file is
//                    compiled with -ffp-contract=off: no FMA). Optionally the per-batch confusion of trainer.py:395-412.
//   vote_predict_k   first maximum over the row widened by a zero column per ignored label (np.insert + np.argmax),
//                    optional reprojection, raw label values out, confusion against raw targets.
//   affine_lrelu_k   LeakyReLU(x * scale[col] + shift[col] (+ addend)): a BatchNorm with frozen statistics.
// No float atomics anywhere: a vote row has exactly one writer per launch (the entry point orders launches when two
// spheres of a batch come from one cloud) and the confusions are counted with integer atomics (LDS, flushed per
// workgroup), which are exact in any order.
#include "common.h"

namespace {

constexpr int VT = 256;          // threads per workgroup
constexpr int VROWS = 128;       // rows of a batch per workgroup (vote update)
constexpr int VC_MAX = 64;       // model classes
constexpr int VL_MAX = 64;       // slots of the full label table (confusion [VL_MAX, VL_MAX] int32 in LDS = 16 KiB)
constexpr int VB_MAX = 4096;     // spheres per batch

template <bool W64>
__device__ __forceinline__ int64_t load_int(const void* p, int64_t i) {
  return W64 ? ((const int64_t*)p)[i] : (int64_t)((const int32_t*)p)[i];
}

// slot of a raw label value in the label table, or -1 (confusion_matrix(labels=...) drops such samples)
__device__ __forceinline__ int slot_of(int64_t value, const int32_t* __restrict__ label_values, int Ctot) {
  for (int s = 0; s < Ctot; ++s)
    if ((int64_t)label_values[s] == value) return s;
  return -1;
}

__device__ __forceinline__ void flush_confusion(const int* s_conf, int Ctot, unsigned long long* conf) {
  for (int e = threadIdx.x; e < Ctot * Ctot; e += blockDim.x) {
    const int v = s_conf[e];
    if (v) atomicAdd(&conf[e], (unsigned long long)v);
  }
}

struct VoteArgs {
  const float* scores;           // [N, C]
  int64_t N;
  int C;
  int is_logits;
  const float* points;           // [N, 3] or NULL
  const int32_t* lengths;        // [B]
  int B;
  const void* input_inds;        // [N]
  const int32_t* cloud_inds;     // [B]
  int n_clouds;
  const int64_t* cloud_offsets;  // [n_clouds + 1] rows
  double* votes;                 // [cloud_offsets[n_clouds], C]
  double smooth, one_minus_smooth;
  float r2_max;
  int b0, b1;                    // spheres [b0, b1) vote in this launch
  // optional per-batch confusion (counted by the launch with do_conf != 0)
  int do_conf;
  const void* labels;            // [N]
  const int32_t* label_values;   // [Ctot]
  const int32_t* col_map;        // [Ctot]
  int Ctot;
  unsigned long long* conf;      // [Ctot, Ctot]
};

template <bool IDX64, bool LAB64>
__global__ __launch_bounds__(VT) void vote_update_k(VoteArgs a) {
  extern __shared__ unsigned char smem[];
  // layout: probabilities [VROWS, C] f32 | destination row [VROWS] int64 | confusion [Ctot, Ctot] int32
  float* sp = (float*)smem;
  int64_t* s_dst = (int64_t*)(smem + (((size_t)VROWS * a.C * sizeof(float) + 7) & ~(size_t)7));
  int* s_conf = (int*)(s_dst + VROWS);
  const int C = a.C;
  const int64_t row0 = (int64_t)blockIdx.x * VROWS;
  const int rows = (int)((a.N - row0) < VROWS ? (a.N - row0) : VROWS);

  if (a.do_conf)
    for (int e = threadIdx.x; e < a.Ctot * a.Ctot; e += VT) s_conf[e] = 0;
  // the tile's scores, read in memory order
  for (int e = threadIdx.x; e < rows * C; e += VT) sp[e] = a.scores[row0 * C + e];
  __syncthreads();

  if ((int)threadIdx.x < rows) {
    const int r = threadIdx.x;
    const int64_t i = row0 + r;
    float* p = sp + r * C;
    if (a.is_logits) {
      float m = p[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, p[c]);
      float s = 0.f;
      for (int c = 0; c < C; ++c) {
        const float e = expf(p[c] - m);
        p[c] = e;
        s += e;
      }
      for (int c = 0; c < C; ++c) p[c] = p[c] / s;
    }
    // which sphere this row belongs to (B is a handful: a scan of the lengths)
    int b = -1;
    int64_t end = 0;
    for (int k = 0; k < a.B; ++k) {
      const int32_t len = a.lengths[k];
      end += len > 0 ? len : 0;
      if (i < end) {
        b = k;
        break;
      }
    }
    int64_t dst = -1;
    if (b >= a.b0 && b < a.b1) {
      bool votes_here = true;
      if (a.points && a.r2_max > 0.f) {
        const float x = a.points[3 * i], y = a.points[3 * i + 1], z = a.points[3 * i + 2];
        const float d2 = (x * x + y * y) + z * z;       // np.sum(points ** 2, axis=1) in float32, no FMA
        votes_here = d2 < a.r2_max;
      }
      const int32_t ci = a.cloud_inds[b];
      if (votes_here && ci >= 0 && ci < a.n_clouds) {
        const int64_t base = a.cloud_offsets[ci], size = a.cloud_offsets[ci + 1] - base;
        const int64_t ind = load_int<IDX64>(a.input_inds, i);
        if (ind >= 0 && ind < size) dst = base + ind;    // an index outside its cloud never writes
      }
    }
    s_dst[r] = dst;
    if (a.do_conf && b >= 0) {
      const int t = slot_of(load_int<LAB64>(a.labels, i), a.label_values, a.Ctot);
      if (t >= 0) {
        int best = 0;
        float bv = a.col_map[0] >= 0 ? p[a.col_map[0]] : 0.f;
        for (int s = 1; s < a.Ctot; ++s) {
          const int col = a.col_map[s];
          const float v = col >= 0 ? p[col] : 0.f;
          if (v > bv) {
            bv = v;
            best = s;
          }
        }
        atomicAdd(&s_conf[t * a.Ctot + best], 1);
      }
    }
  }
  __syncthreads();

  for (int e = threadIdx.x; e < rows * C; e += VT) {
    const int r = e / C;
    const int64_t dst = s_dst[r];
    if (dst < 0) continue;
    double* v = a.votes + dst * C + (e - r * C);
    const double kept = a.smooth * *v;
    const double added = a.one_minus_smooth * (double)sp[e];
    *v = kept + added;
  }
  if (a.do_conf) flush_confusion(s_conf, a.Ctot, a.conf);
}

template <bool P64>
__global__ __launch_bounds__(VT) void vote_predict_k(const double* __restrict__ votes, int64_t Nc, int C, const void* proj,
                                                     int64_t Nfull, const int32_t* __restrict__ label_values,
                                                     const int32_t* __restrict__ col_map, int Ctot,
                                                     const int32_t* __restrict__ targets, int32_t* __restrict__ preds,
                                                     unsigned long long* conf) {
  __shared__ int s_conf[VL_MAX * VL_MAX];
  __shared__ int s_lab[VL_MAX], s_col[VL_MAX];
  const bool count = targets != nullptr && conf != nullptr;
  if (count)
    for (int e = threadIdx.x; e < Ctot * Ctot; e += VT) s_conf[e] = 0;
  if ((int)threadIdx.x < Ctot) {
    s_lab[threadIdx.x] = label_values[threadIdx.x];
    const int col = col_map[threadIdx.x];
    s_col[threadIdx.x] = (col >= 0 && col < C) ? col : -1;
  }
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * VT + threadIdx.x;
  if (j < Nfull) {
    const int64_t src = proj ? load_int<P64>(proj, j) : j;
    if (src >= 0 && src < Nc) {
      const double* row = votes + src * C;
      int best = 0;
      double bv = s_col[0] >= 0 ? row[s_col[0]] : 0.0;
      for (int s = 1; s < Ctot; ++s) {
        const double v = s_col[s] >= 0 ? row[s_col[s]] : 0.0;
        if (v > bv) {                                   // first maximum, like np.argmax
          bv = v;
          best = s;
        }
      }
      preds[j] = s_lab[best];
      if (count) {
        const int32_t tv = targets[j];
        int t = -1;
        for (int s = 0; s < Ctot; ++s)
          if (s_lab[s] == tv) {
            t = s;
            break;
          }
        if (t >= 0) atomicAdd(&s_conf[t * Ctot + best], 1);
      }
    } else {
      preds[j] = -1;                                    // a reprojection index outside the cloud: no prediction, not counted
    }
  }
  __syncthreads();
  if (count) flush_confusion(s_conf, Ctot, conf);
}

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

template <bool ADD>
__global__ __launch_bounds__(VT) void affine_lrelu_k(const float* __restrict__ x, const float* __restrict__ scale,
                                                     const float* __restrict__ shift, const float* __restrict__ addend,
                                                     int64_t total, int C, float slope, float* __restrict__ y) {
  const int64_t e = (int64_t)blockIdx.x * VT + threadIdx.x;
  if (e >= total) return;
  const int c = (int)(e % C);
  float v = x[e] * scale[c] + shift[c];
  if (ADD) v += addend[e];
  y[e] = lrelu(v, slope);
}

// C % 4 == 0 and 16-byte aligned operands: four columns of one row per thread
template <bool ADD>
__global__ __launch_bounds__(VT) void affine_lrelu_v4_k(const float4* __restrict__ x, const float4* __restrict__ scale,
                                                        const float4* __restrict__ shift, const float4* __restrict__ addend,
                                                        int64_t total4, int C4, float slope, float4* __restrict__ y) {
  const int64_t e = (int64_t)blockIdx.x * VT + threadIdx.x;
  if (e >= total4) return;
  const int c = (int)(e % C4);
  const float4 a = x[e], s = scale[c], t = shift[c];
  float4 v;
  v.x = a.x * s.x + t.x;
  v.y = a.y * s.y + t.y;
  v.z = a.z * s.z + t.z;
  v.w = a.w * s.w + t.w;
  if (ADD) {
    const float4 d = addend[e];
    v.x += d.x;
    v.y += d.y;
    v.z += d.z;
    v.w += d.w;
  }
  v.x = lrelu(v.x, slope);
  v.y = lrelu(v.y, slope);
  v.z = lrelu(v.z, slope);
  v.w = lrelu(v.w, slope);
  y[e] = v;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mvk_vote_update(const float* scores, int64_t N, int C, int is_logits, const float* points,
                               const int32_t* lengths, int B, const void* input_inds, int inds64,
                               const int32_t* cloud_inds, const int32_t* cloud_inds_host, int n_clouds,
                               const int64_t* cloud_offsets, double* votes, double smooth, double one_minus_smooth,
                               float r2_max, const void* labels, int labels64, const int32_t* label_values,
                               const int32_t* col_map, int Ctot, int64_t* confusion, void* stream) {
  MVK_REQUIRE(N >= 0 && C > 0 && C <= VC_MAX && B > 0 && B <= VB_MAX && n_clouds > 0,
              "vote_update: bad sizes N=%lld C=%d (<= %d) B=%d (<= %d) clouds=%d", (long long)N, C, VC_MAX, B, VB_MAX,
              n_clouds);
  MVK_REQUIRE(N < ((int64_t)1 << 31) * VROWS, "vote_update: too many rows");
  if (N == 0) return 0;
  MVK_REQUIRE(scores && lengths && input_inds && cloud_inds && cloud_inds_host && cloud_offsets && votes,
              "vote_update: null operand");
  const bool do_conf = confusion != nullptr;
  if (do_conf) {
    MVK_REQUIRE(labels && label_values && col_map && Ctot > 0 && Ctot <= VL_MAX,
                "vote_update: the confusion needs labels, label_values, col_map and 0 < Ctot <= %d (got %d)", VL_MAX, Ctot);
  }
  VoteArgs a;
  a.scores = scores;
  a.N = N;
  a.C = C;
  a.is_logits = is_logits;
  a.points = points;
  a.lengths = lengths;
  a.B = B;
  a.input_inds = input_inds;
  a.cloud_inds = cloud_inds;
  a.n_clouds = n_clouds;
  a.cloud_offsets = cloud_offsets;
  a.votes = votes;
  a.smooth = smooth;
  a.one_minus_smooth = one_minus_smooth;
  a.r2_max = r2_max;
  a.labels = labels;
  a.label_values = label_values;
  a.col_map = col_map;
  a.Ctot = do_conf ? Ctot : 0;
  a.conf = (unsigned long long*)confusion;
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)cdiv64(N, VROWS);
  const size_t lds = (((size_t)VROWS * C * sizeof(float) + 7) & ~(size_t)7) + VROWS * sizeof(int64_t) +
                     (size_t)a.Ctot * a.Ctot * sizeof(int);
  // Spheres are applied in batch order (tester.py:171-186). Within one launch every vote row has one writer only if
  // the launch's spheres come from pairwise different clouds: cut the batch into such runs, one launch each, in order.
  int b0 = 0;
  bool first = true;
  while (b0 < B) {
    int b1 = b0 + 1;
    for (; b1 < B; ++b1) {
      bool seen = false;
      for (int k = b0; k < b1 && !seen; ++k) seen = cloud_inds_host[k] == cloud_inds_host[b1];
      if (seen) break;
    }
    a.b0 = b0;
    a.b1 = b1;
    a.do_conf = (do_conf && first) ? 1 : 0;
    if (inds64) {
      if (labels64)
        hipLaunchKernelGGL((vote_update_k<true, true>), dim3(gx), dim3(VT), lds, st, a);
      else
        hipLaunchKernelGGL((vote_update_k<true, false>), dim3(gx), dim3(VT), lds, st, a);
    } else {
      if (labels64)
        hipLaunchKernelGGL((vote_update_k<false, true>), dim3(gx), dim3(VT), lds, st, a);
      else
        hipLaunchKernelGGL((vote_update_k<false, false>), dim3(gx), dim3(VT), lds, st, a);
    }
    MVK_CHECK_HIP(hipGetLastError());
    first = false;
    b0 = b1;
  }
  return 0;
}

extern "C" int mvk_vote_predict(const double* votes, int64_t Nc, int C, const void* proj, int proj64, int64_t Nfull,
                                const int32_t* label_values, const int32_t* col_map, int Ctot, const int32_t* targets,
                                int32_t* preds, int64_t* confusion, void* stream) {
  MVK_REQUIRE(Nc >= 0 && Nfull >= 0 && C > 0 && C <= VC_MAX && Ctot > 0 && Ctot <= VL_MAX,
              "vote_predict: bad sizes Nc=%lld Nfull=%lld C=%d (<= %d) Ctot=%d (<= %d)", (long long)Nc, (long long)Nfull, C,
              VC_MAX, Ctot, VL_MAX);
  MVK_REQUIRE(proj || Nfull == Nc, "vote_predict: without a reprojection Nfull must equal Nc");
  MVK_REQUIRE(Nfull < ((int64_t)1 << 31) * VT, "vote_predict: too many rows");
  if (Nfull == 0) return 0;
  MVK_REQUIRE(votes && label_values && col_map && preds, "vote_predict: null operand");
  MVK_REQUIRE((targets == nullptr) == (confusion == nullptr), "vote_predict: targets and confusion go together");
  hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)cdiv64(Nfull, VT);
  if (proj64)
    hipLaunchKernelGGL(vote_predict_k<true>, dim3(gx), dim3(VT), 0, st, votes, Nc, C, proj, Nfull, label_values, col_map,
                       Ctot, targets, preds, (unsigned long long*)confusion);
  else
    hipLaunchKernelGGL(vote_predict_k<false>, dim3(gx), dim3(VT), 0, st, votes, Nc, C, proj, Nfull, label_values, col_map,
                       Ctot, targets, preds, (unsigned long long*)confusion);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_affine_lrelu(const float* x, const float* scale, const float* shift, const float* addend, int64_t R,
                                int C, float slope, float* y, void* stream) {
  MVK_REQUIRE(R >= 0 && C > 0, "affine_lrelu: bad sizes R=%lld C=%d", (long long)R, C);
  if (R == 0) return 0;
  MVK_REQUIRE(x && scale && shift && y, "affine_lrelu: null operand");
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = R * C;
  MVK_REQUIRE(total < ((int64_t)1 << 31) * VT, "affine_lrelu: too many elements");
  const bool v4 = C % 4 == 0 && aligned16(x) && aligned16(scale) && aligned16(shift) && aligned16(y) &&
                  (!addend || aligned16(addend));
  if (v4) {
    const unsigned gx = (unsigned)cdiv64(total / 4, VT);
    if (addend)
      hipLaunchKernelGGL(affine_lrelu_v4_k<true>, dim3(gx), dim3(VT), 0, st, (const float4*)x, (const float4*)scale,
                         (const float4*)shift, (const float4*)addend, total / 4, C / 4, slope, (float4*)y);
    else
      hipLaunchKernelGGL(affine_lrelu_v4_k<false>, dim3(gx), dim3(VT), 0, st, (const float4*)x, (const float4*)scale,
                         (const float4*)shift, (const float4*)nullptr, total / 4, C / 4, slope, (float4*)y);
  } else {
    const unsigned gx = (unsigned)cdiv64(total, VT);
    if (addend)
      hipLaunchKernelGGL(affine_lrelu_k<true>, dim3(gx), dim3(VT), 0, st, x, scale, shift, addend, total, C, slope, y);
    else
      hipLaunchKernelGGL(affine_lrelu_k<false>, dim3(gx), dim3(VT), 0, st, x, scale, shift, (const float*)nullptr, total, C,
                         slope, y);
  }
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
