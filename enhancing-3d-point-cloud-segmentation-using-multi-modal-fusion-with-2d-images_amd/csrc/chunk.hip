// The MVPNet baseline's whole-scene test on the device (reference: mvpnet/utils/chunk_util.py:4-53,
// mvpnet/test_mvpnet_3d.py:141-178, mvpnet/evaluate_3d.py:19-36).
//
// The reference cuts a scene into sliding xy chunks with a Python loop over the chunk corners (two full-N boolean masks
// per corner), copies every chunk's logits to the host and adds them into a per-point array with NumPy fancy indexing.
// Here the scene stays in HBM:
//   box_count_k        points inside each of n xy boxes, all boxes in one launch. Membership is
//                      (double)x >= x_lo && (double)x <= x_hi (and the same for y), both ends inclusive, in float64.
//   box_block_count_k / box_scan_k / box_scatter_k
//                      the members of every kept box in ascending index order (np.nonzero order) as one CSR, with the
//                      ordered compaction of compact.h: per-block ballot counts, a scan of the block counts per box,
//                      a scatter at block offset + rank.
//   box_zrange_k       float32 min / max of z over each box's members (one workgroup per box reads its CSR row).
//   chunk_vote_add_k   sums[chunk_ind[j], c] += logits[c, j], counts[chunk_ind[j]] += 1: a 64-column tile of the
//                      channel-major logits is transposed through LDS, so the reads run along columns and the writes
//                      along rows. Plain read-add-write: the indices of one chunk are distinct, chunks follow each other
//                      in stream order, so the float32 sums are those of the reference's loop bit for bit.
//   chunk_vote_finish_k  mean = sums / max(counts, 1) as a float32 division, first maximum, C where a point was never
//                      visited, optional confusion against labels.
// No float atomics. Integer counters are summed in LDS first and leave a workgroup as one atomic per counter. Box bounds
// are read with wave-uniform addresses (scalar loads). Compiled with -ffp-contract=off like the other geometry files.
#include <limits>

#include "common.h"
#include "compact.h"

namespace {

constexpr int BC_G = 256;        // boxes per LDS group of the count kernel
constexpr int BS_G = 64;         // boxes per LDS group of the select kernels ([BS_G, COMPACT_WAVES] wave counts)
constexpr int ZT = 256;          // threads of the z-range kernel
constexpr int CV_T = 256;        // threads of the vote kernels
constexpr int CV_COLS = 64;      // chunk columns per workgroup (vote add)
constexpr int CV_ROWS = 128;     // scene rows per workgroup (finish)
constexpr int CV_C_MAX = 64;     // classes

__device__ __forceinline__ bool in_box(double x, double y, const double* __restrict__ box) {
  return x >= box[0] && y >= box[1] && x <= box[2] && y <= box[3];
}

__global__ __launch_bounds__(COMPACT_T) void box_count_k(const float* __restrict__ pts, int64_t N,
                                                         const double* __restrict__ boxes, int n,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ int s_cnt[BC_G];
  const int64_t i = (int64_t)blockIdx.x * COMPACT_T + threadIdx.x;
  const bool valid = i < N;
  const double x = valid ? (double)pts[i * 3] : 0.0, y = valid ? (double)pts[i * 3 + 1] : 0.0;
  const int lane = threadIdx.x & 63;
  for (int g0 = 0; g0 < n; g0 += BC_G) {
    const int ng = n - g0 < BC_G ? n - g0 : BC_G;
    if ((int)threadIdx.x < ng) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int g = 0; g < ng; ++g) {
      const unsigned long long m = __ballot(valid && in_box(x, y, boxes + (int64_t)(g0 + g) * 4));
      if (lane == 0 && m) atomicAdd(&s_cnt[g], __popcll(m));
    }
    __syncthreads();
    if ((int)threadIdx.x < ng && s_cnt[threadIdx.x])
      atomicAdd(&counts[g0 + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    __syncthreads();
  }
}

// s_wc[g, w] = members of box g0 + g in wave w of this block, for the ng boxes of one group
__device__ __forceinline__ void box_wave_counts(bool valid, double x, double y, const double* __restrict__ boxes, int g0,
                                                int ng, int* s_wc) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int g = 0; g < ng; ++g) {
    const unsigned long long m = __ballot(valid && in_box(x, y, boxes + (int64_t)(g0 + g) * 4));
    if (lane == 0) s_wc[g * COMPACT_WAVES + w] = __popcll(m);
  }
}

// block_count [n, nblk]: members of box b among the points of block k
__global__ __launch_bounds__(COMPACT_T) void box_block_count_k(const float* __restrict__ pts, int64_t N,
                                                               const double* __restrict__ boxes, int n,
                                                               int* __restrict__ block_count) {
  __shared__ int s_wc[BS_G * COMPACT_WAVES];
  const int64_t i = (int64_t)blockIdx.x * COMPACT_T + threadIdx.x;
  const bool valid = i < N;
  const double x = valid ? (double)pts[i * 3] : 0.0, y = valid ? (double)pts[i * 3 + 1] : 0.0;
  for (int g0 = 0; g0 < n; g0 += BS_G) {
    const int ng = n - g0 < BS_G ? n - g0 : BS_G;
    box_wave_counts(valid, x, y, boxes, g0, ng, s_wc);
    __syncthreads();
    if ((int)threadIdx.x < ng)
      block_count[(int64_t)(g0 + threadIdx.x) * gridDim.x + blockIdx.x] =
          compact_wave_offset(s_wc + threadIdx.x * COMPACT_WAVES, COMPACT_WAVES);
    __syncthreads();
  }
}

// one workgroup per box: its row of block counts becomes block offsets
__global__ __launch_bounds__(COMPACT_T) void box_scan_k(int* __restrict__ block_count, int nblk) {
  __shared__ int carry;
  __shared__ int ws[COMPACT_WAVES];
  compact_scan_counts(block_count + (int64_t)blockIdx.x * nblk, nblk, &carry, ws);
}

__global__ __launch_bounds__(COMPACT_T) void box_scatter_k(const float* __restrict__ pts, int64_t N,
                                                           const double* __restrict__ boxes, int n,
                                                           const int* __restrict__ block_off,
                                                           const int64_t* __restrict__ offsets, int64_t total,
                                                           int64_t* __restrict__ idx) {
  __shared__ int s_wc[BS_G * COMPACT_WAVES];
  const int64_t i = (int64_t)blockIdx.x * COMPACT_T + threadIdx.x;
  const bool valid = i < N;
  const double x = valid ? (double)pts[i * 3] : 0.0, y = valid ? (double)pts[i * 3 + 1] : 0.0;
  const int w = threadIdx.x >> 6;
  for (int g0 = 0; g0 < n; g0 += BS_G) {
    const int ng = n - g0 < BS_G ? n - g0 : BS_G;
    box_wave_counts(valid, x, y, boxes, g0, ng, s_wc);
    __syncthreads();
    for (int g = 0; g < ng; ++g) {
      const int b = g0 + g;
      const int64_t lo = offsets[b], hi = offsets[b + 1];              // wave-uniform, like the bounds: scalar loads
      const int in_front = block_off[(int64_t)b * gridDim.x + blockIdx.x];
      const bool hit = valid && in_box(x, y, boxes + (int64_t)b * 4);
      const unsigned long long m = __ballot(hit);
      if (!hit) continue;
      const int64_t pos = lo + in_front + compact_wave_offset(s_wc + g * COMPACT_WAVES, w) + compact_lane_rank(m);
      // offsets that do not belong to these boxes never make a write leave the box's row or the buffer
      if (pos >= lo && pos < hi && pos >= 0 && pos < total) idx[pos] = i;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(ZT) void box_zrange_k(const float* __restrict__ pts, int64_t N,
                                                   const int64_t* __restrict__ offsets, int64_t total,
                                                   const int64_t* __restrict__ idx, float* __restrict__ zmin,
                                                   float* __restrict__ zmax) {
  __shared__ float s_lo[ZT / 64], s_hi[ZT / 64];
  const int b = blockIdx.x;
  int64_t j0 = offsets[b], j1 = offsets[b + 1];
  if (j0 < 0) j0 = 0;
  if (j1 > total) j1 = total;
  float lo = std::numeric_limits<float>::infinity(), hi = -std::numeric_limits<float>::infinity();
  for (int64_t j = j0 + threadIdx.x; j < j1; j += ZT) {
    const int64_t i = idx[j];
    if (i < 0 || i >= N) continue;
    const float z = pts[i * 3 + 2];
    lo = fminf(lo, z);
    hi = fmaxf(hi, z);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < ZT / 64; ++k) {
      lo = fminf(lo, s_lo[k]);
      hi = fmaxf(hi, s_hi[k]);
    }
    zmin[b] = lo;
    zmax[b] = hi;
  }
}

// ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int lds_stride(int C) { return C | 1; }       // odd: column reads of the tile hit 32 banks

__global__ __launch_bounds__(CV_T) void chunk_vote_add_k(const float* __restrict__ logits, int C, int64_t ld,
                                                         const int64_t* __restrict__ chunk_ind, int64_t n,
                                                         float* __restrict__ sums, int32_t* __restrict__ counts,
                                                         int64_t N) {
  __shared__ float s_tile[CV_COLS * (CV_C_MAX + 1)];
  __shared__ int64_t s_row[CV_COLS];
  const int64_t j0 = (int64_t)blockIdx.x * CV_COLS;
  const int cols = (int)(n - j0 < CV_COLS ? n - j0 : CV_COLS);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, S = lds_stride(C);
  if ((int)threadIdx.x < CV_COLS) {
    int64_t r = -1;
    if ((int)threadIdx.x < cols) {
      r = chunk_ind[j0 + threadIdx.x];
      if (r < 0 || r >= N) r = -1;                      // an index outside the scene writes nothing
    }
    s_row[threadIdx.x] = r;
    if (r >= 0) counts[r] += 1;
  }
  if (lane < cols)
    for (int c = w; c < C; c += CV_T / 64) s_tile[lane * S + c] = logits[(int64_t)c * ld + j0 + lane];
  __syncthreads();
  for (int e = threadIdx.x; e < cols * C; e += CV_T) {
    const int j = e / C, c = e - j * C;
    const int64_t r = s_row[j];
    if (r >= 0) sums[r * C + c] += s_tile[j * S + c];
  }
}

__device__ __forceinline__ void flush_counts(const int* s_conf, int C, unsigned long long* conf) {
  for (int e = threadIdx.x; e < C * C; e += blockDim.x) {
    const int v = s_conf[e];
    if (v) atomicAdd(&conf[e], (unsigned long long)v);
  }
}

// a pair counts when truth and prediction are both one of 0..C-1 (confusion_matrix(labels=arange(C)))
__device__ __forceinline__ void count_pair(int64_t truth, int64_t pred, int C, int* s_conf) {
  if (truth >= 0 && truth < C && pred >= 0 && pred < C) atomicAdd(&s_conf[(int)truth * C + (int)pred], 1);
}

// mean may be sums: every element is read and written by one thread
__global__ __launch_bounds__(CV_T) void chunk_vote_finish_k(const float* sums, const int32_t* __restrict__ counts,
                                                            int64_t N, int C, float* mean, int64_t* __restrict__ pred,
                                                            const int64_t* __restrict__ labels,
                                                            unsigned long long* conf) {
  extern __shared__ unsigned char smem[];
  // layout: means [CV_ROWS, C | 1] f32 | visit counts [CV_ROWS] int32 | confusion [C, C] int32
  const int S = lds_stride(C);
  float* s_tile = (float*)smem;
  int* s_cnt = (int*)(s_tile + CV_ROWS * S);
  int* s_conf = s_cnt + CV_ROWS;
  const bool count = labels != nullptr && conf != nullptr;
  const int64_t row0 = (int64_t)blockIdx.x * CV_ROWS;
  const int rows = (int)(N - row0 < CV_ROWS ? N - row0 : CV_ROWS);
  if (count)
    for (int e = threadIdx.x; e < C * C; e += CV_T) s_conf[e] = 0;
  if ((int)threadIdx.x < rows) s_cnt[threadIdx.x] = counts[row0 + threadIdx.x];
  __syncthreads();
  for (int e = threadIdx.x; e < rows * C; e += CV_T) {
    const int r = e / C, c = e - r * C;
    const int visits = s_cnt[r];
    const float m = sums[row0 * C + e] / (float)(visits > 1 ? visits : 1);      // IEEE division, not a reciprocal product
    mean[row0 * C + e] = m;
    s_tile[r * S + c] = m;
  }
  __syncthreads();
  if ((int)threadIdx.x < rows) {
    const float* row = s_tile + threadIdx.x * S;
    int best = 0;
    float bv = row[0];
    for (int c = 1; c < C; ++c)
      if (row[c] > bv) {                                 // first maximum, like np.argmax
        bv = row[c];
        best = c;
      }
    const int64_t p = s_cnt[threadIdx.x] == 0 ? C : best;
    pred[row0 + threadIdx.x] = p;
    if (count) count_pair(labels[row0 + threadIdx.x], p, C, s_conf);
  }
  __syncthreads();
  if (count) flush_counts(s_conf, C, conf);
}

// a bounded grid strides over the pairs, so the C x C table is zeroed and flushed once per workgroup, not once per 256 pairs
__global__ __launch_bounds__(CV_T) void chunk_confusion_k(const int64_t* __restrict__ pred,
                                                          const int64_t* __restrict__ labels, int64_t N, int C,
                                                          unsigned long long* conf) {
  __shared__ int s_conf[CV_C_MAX * CV_C_MAX];
  for (int e = threadIdx.x; e < C * C; e += CV_T) s_conf[e] = 0;
  __syncthreads();
  const int64_t step = (int64_t)gridDim.x * CV_T;
  for (int64_t i = (int64_t)blockIdx.x * CV_T + threadIdx.x; i < N; i += step) count_pair(labels[i], pred[i], C, s_conf);
  __syncthreads();
  flush_counts(s_conf, C, conf);
}

constexpr int CONF_MAX_GRID = 1024;     // 4 workgroups per CU: an int32 LDS counter holds a workgroup's share of any N < 2^40

constexpr int64_t MAX_GRID = ((int64_t)1 << 31) - 1;

}  // namespace

extern "C" int mvk_box_count(const float* pts, int64_t N, const double* boxes, int n, int64_t* counts, void* stream) {
  MVK_REQUIRE(N >= 0 && n >= 0 && cdiv64(N, COMPACT_T) <= MAX_GRID, "box_count: bad sizes N=%lld n=%d", (long long)N, n);
  if (n == 0) return 0;
  MVK_REQUIRE(boxes && counts && (pts || N == 0), "box_count: null operand");
  hipStream_t st = (hipStream_t)stream;
  MVK_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int64_t), st));
  if (N == 0) return 0;
  hipLaunchKernelGGL(box_count_k, dim3((unsigned)cdiv64(N, COMPACT_T)), dim3(COMPACT_T), 0, st, pts, N, boxes, n,
                     (unsigned long long*)counts);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t mvk_box_select_workspace(int64_t N, int n) {
  return cdiv64(N > 0 ? N : 1, COMPACT_T) * (int64_t)(n > 0 ? n : 1) * (int64_t)sizeof(int) + 64;
}

extern "C" int mvk_box_select(const float* pts, int64_t N, const double* boxes, int n, const int64_t* offsets,
                              int64_t total, int64_t* idx, float* zmin, float* zmax, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  MVK_REQUIRE(N >= 0 && n >= 0 && total >= 0 && cdiv64(N, COMPACT_T) <= MAX_GRID, "box_select: bad sizes N=%lld n=%d total=%lld",
              (long long)N, n, (long long)total);
  if (n == 0) return 0;
  MVK_REQUIRE(boxes && offsets && (idx || total == 0) && (pts || N == 0), "box_select: null operand");
  MVK_REQUIRE((zmin == nullptr) == (zmax == nullptr), "box_select: zmin and zmax go together");
  MVK_REQUIRE(workspace && workspace_bytes >= mvk_box_select_workspace(N, n), "box_select: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (N > 0 && total > 0) {
    const int nblk = (int)cdiv64(N, COMPACT_T);
    int* bc = (int*)workspace;
    hipLaunchKernelGGL(box_block_count_k, dim3(nblk), dim3(COMPACT_T), 0, st, pts, N, boxes, n, bc);
    MVK_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(box_scan_k, dim3(n), dim3(COMPACT_T), 0, st, bc, nblk);
    MVK_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(box_scatter_k, dim3(nblk), dim3(COMPACT_T), 0, st, pts, N, boxes, n, (const int*)bc, offsets, total,
                       idx);
    MVK_CHECK_HIP(hipGetLastError());
  }
  if (zmin) {
    hipLaunchKernelGGL(box_zrange_k, dim3(n), dim3(ZT), 0, st, pts, N, offsets, total, (const int64_t*)idx, zmin, zmax);
    MVK_CHECK_HIP(hipGetLastError());
  }
  return 0;
}

extern "C" int mvk_chunk_vote_add(const float* logits, int C, int64_t ld, const int64_t* chunk_ind, int64_t n, float* sums,
                                  int32_t* counts, int64_t N, void* stream) {
  MVK_REQUIRE(C > 0 && C <= CV_C_MAX && n >= 0 && ld >= n && N >= 0 && cdiv64(n, CV_COLS) <= MAX_GRID,
              "chunk_vote_add: bad sizes C=%d (<= %d) n=%lld ld=%lld (>= n) N=%lld", C, CV_C_MAX, (long long)n, (long long)ld,
              (long long)N);
  if (n == 0 || N == 0) return 0;
  MVK_REQUIRE(logits && chunk_ind && sums && counts, "chunk_vote_add: null operand");
  hipLaunchKernelGGL(chunk_vote_add_k, dim3((unsigned)cdiv64(n, CV_COLS)), dim3(CV_T), 0, (hipStream_t)stream, logits, C, ld,
                     chunk_ind, n, sums, counts, N);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_chunk_vote_finish(const float* sums, const int32_t* counts, int64_t N, int C, float* mean, int64_t* pred,
                                     const int64_t* labels, int64_t* confusion, void* stream) {
  MVK_REQUIRE(C > 0 && C <= CV_C_MAX && N >= 0 && cdiv64(N, CV_ROWS) <= MAX_GRID, "chunk_vote_finish: bad sizes N=%lld C=%d (<= %d)",
              (long long)N, C, CV_C_MAX);
  MVK_REQUIRE((labels == nullptr) == (confusion == nullptr), "chunk_vote_finish: labels and confusion go together");
  if (N == 0) return 0;
  MVK_REQUIRE(sums && counts && mean && pred, "chunk_vote_finish: null operand");
  const size_t lds = (size_t)CV_ROWS * (C | 1) * sizeof(float) + CV_ROWS * sizeof(int) + (size_t)C * C * sizeof(int);
  hipLaunchKernelGGL(chunk_vote_finish_k, dim3((unsigned)cdiv64(N, CV_ROWS)), dim3(CV_T), lds, (hipStream_t)stream, sums,
                     counts, N, C, mean, pred, labels, (unsigned long long*)confusion);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_chunk_confusion(const int64_t* pred, const int64_t* labels, int64_t N, int C, int64_t* confusion,
                                   void* stream) {
  MVK_REQUIRE(C > 0 && C <= CV_C_MAX && N >= 0 && N < ((int64_t)1 << 40), "chunk_confusion: bad sizes N=%lld C=%d (<= %d)",
              (long long)N, C, CV_C_MAX);
  if (N == 0) return 0;
  MVK_REQUIRE(pred && labels && confusion, "chunk_confusion: null operand");
  const int64_t want = cdiv64(N, CV_T);
  hipLaunchKernelGGL(chunk_confusion_k, dim3((unsigned)(want < CONF_MAX_GRID ? want : CONF_MAX_GRID)), dim3(CV_T), 0, (hipStream_t)stream, pred, labels, N,
                     C, (unsigned long long*)confusion);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
