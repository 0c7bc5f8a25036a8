// PointNet++ set abstraction in TRAINING mode on the library's GEMM and BatchNorm: the two ends of the
// shared MLP that the products and bn_lrelu do not cover, each with its backward.
//
//   sa_rows_fwd_k      the input rows of the shared MLP as the channel-major operand X [Cin, R], R = B*M*K, row
//                      r = (b*M + m)*K + k = [feature[b, :, j] | xyz[b, :, j] - new_xyz[b, :, m]], j = index[b, m, k]
//                      (QueryGrouper's order; -ffp-contract=off: the subtraction is one rounding). Lanes run along r:
//                      the index read and every store are coalesced, each gathered 4-byte read stays inside one channel
//                      plane of N floats (L2 resident), as in group_points_fwd_kernel and fa_gather_kernel.
//   sa_rows_bwd_k      dfeature[b, c, j] += dX[c, r]: float atomics onto a zeroed buffer (the default mode).
//   sa_rows_bwd_csr_k  the same sums as a per-key gather over the transposed index (mvk_index_csr, pn2_ordered.hip): a
//                      lane per key, acc = fl(acc + g) over the key's positions in ascending order, every element of
//                      dfeature written (+0 without entries). ordered_bwd_k's walk on the operand's [Cin, B, L] layout.
//   rows_max_fwd_k     Y [R, Cout] row-major (what bn_lrelu returns) -> out / arg [B, Cout, M]: the maximum over the K rows
//                      of a centroid and the smallest k attaining it. A workgroup owns MAX_TM centroids x MAX_TC channels:
//                      lanes along channels while reading (256-byte segments of a row), a padded LDS tile, lanes along M
//                      while storing (128-byte segments of a channel plane).
//   rows_max_bwd_k     g, arg [B, Cout, M] -> dY [R, Cout]: the same tile the other way round; every element of dY is
//                      written (g at arg, +0 elsewhere), no zero fill, no atomics.
// No kernel reads anything back; grids are fixed by the sizes: all five are capturable.
#include "common.h"

namespace {

constexpr int64_t ROWS_LIMIT = (int64_t)1 << 31;
constexpr int ROWS_T = 256;
constexpr int ROWS_CH = 8;          // channels per lane of sa_rows_bwd_csr_k
constexpr int MAX_T = 256;
constexpr int MAX_TM = 32;          // centroids per tile
constexpr int MAX_TC = 64;          // channels per tile
constexpr int MAX_PAD = MAX_TM + 1; // odd stride: ds_write of a wave (lanes along channels) hits 32 distinct banks per half

// grid (ceil(R / 256), channel groups): every group strides over the feature channels, group 0 also writes the coordinates
__global__ __launch_bounds__(ROWS_T) void sa_rows_fwd_k(const float* __restrict__ xyz, const float* __restrict__ feature,
                                                        const float* __restrict__ new_xyz,
                                                        const int64_t* __restrict__ index, int C, int use_xyz, int64_t N,
                                                        int64_t M, int64_t K, int64_t R, float* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * ROWS_T + threadIdx.x;
  if (e >= R) return;
  const int64_t j = index[e];
  const bool ok = j >= 0 && j < N;
  const int64_t bm = e / K, b = bm / M;
  const float* f = feature + b * C * N + (ok ? j : 0);
  for (int c = blockIdx.y; c < C; c += gridDim.y) X[(int64_t)c * R + e] = ok ? f[(int64_t)c * N] : 0.f;
  if (use_xyz && blockIdx.y == 0) {
    const int64_t m = bm - b * M;
    const float* p = xyz + b * 3 * N + (ok ? j : 0);
    const float* q = new_xyz + b * 3 * M + m;
#pragma unroll
    for (int d = 0; d < 3; ++d) X[(int64_t)(C + d) * R + e] = (ok ? p[d * N] : 0.f) - q[d * M];
  }
}

// one lane per (feature channel, row)
__global__ __launch_bounds__(ROWS_T) void sa_rows_bwd_k(const float* __restrict__ dX, const int64_t* __restrict__ index,
                                                        int C, int64_t N, int64_t L, int64_t R,
                                                        float* __restrict__ dfeature) {
  const int64_t t = (int64_t)blockIdx.x * ROWS_T + threadIdx.x;
  if (t >= (int64_t)C * R) return;
  const int64_t c = t / R, e = t - c * R;
  const int64_t j = index[e];
  if (j >= 0 && j < N) atomicAdd(dfeature + ((e / L) * C + c) * N + j, dX[t]);
}

// one workgroup = 256 keys x ROWS_CH channels of one batch element (ordered_bwd_k, pn2_ordered.hip)
__global__ __launch_bounds__(ROWS_T) void sa_rows_bwd_csr_k(const float* __restrict__ dX,
                                                            const int32_t* __restrict__ row_start,
                                                            const int32_t* __restrict__ entries, int C, int64_t N,
                                                            int64_t L, int64_t R, int nchunk, int nkeyblk,
                                                            float* __restrict__ dfeature) {
  const int kb = blockIdx.x % nkeyblk;
  const int bc = blockIdx.x / nkeyblk;
  const int chunk = bc % nchunk;
  const int64_t b = bc / nchunk;
  const int64_t j = (int64_t)kb * ROWS_T + threadIdx.x;
  if (j >= N) return;
  const int c0 = chunk * ROWS_CH;
  const float* gp[ROWS_CH];
#pragma unroll
  for (int u = 0; u < ROWS_CH; ++u) {
    const int c = c0 + u < C ? c0 + u : C - 1;                           // a chunk's surplus lanes re-read the last channel
    gp[u] = dX + (int64_t)c * R + b * L;
  }
  float acc[ROWS_CH];
#pragma unroll
  for (int u = 0; u < ROWS_CH; ++u) acc[u] = 0.f;
  int64_t beg = row_start[b * N + j], end = row_start[b * N + j + 1];
  if (beg < 0) beg = 0;
  if (end > R) end = R;
  for (int64_t i = beg; i < end; ++i) {
    const int64_t p = entries[i];
    if (p < 0 || p >= L) continue;
#pragma unroll
    for (int u = 0; u < ROWS_CH; ++u) acc[u] = acc[u] + gp[u][p];
  }
#pragma unroll
  for (int u = 0; u < ROWS_CH; ++u)
    if (c0 + u < C) dfeature[(b * C + c0 + u) * N + j] = acc[u];
}

// blockIdx.x = (b * tiles_m + tile_m) * tiles_c + tile_c
__global__ __launch_bounds__(MAX_T) void rows_max_fwd_k(const float* __restrict__ Y, int64_t M, int64_t K, int Cout,
                                                        int tiles_m, int tiles_c, float* __restrict__ out,
                                                        int32_t* __restrict__ arg) {
  __shared__ float s_val[MAX_TC][MAX_PAD];
  __shared__ int32_t s_arg[MAX_TC][MAX_PAD];
  const int tile_c = blockIdx.x % tiles_c;
  const int64_t bt = blockIdx.x / tiles_c;
  const int64_t b = bt / tiles_m, m0 = (bt % tiles_m) * MAX_TM;
  const int c0 = tile_c * MAX_TC;
  {
    const int tc = threadIdx.x & (MAX_TC - 1);
    const int c = c0 + tc;
    for (int mi = threadIdx.x / MAX_TC; mi < MAX_TM; mi += MAX_T / MAX_TC) {
      const int64_t m = m0 + mi;
      if (c >= Cout || m >= M) continue;
      const float* y = Y + ((b * M + m) * K) * Cout + c;
      float best = y[0];
      int32_t at = 0;
      for (int64_t k = 1; k < K; ++k) {
        const float v = y[k * Cout];
        if (v > best || (v != v && best == best)) {                      // strict: the smallest k; the first NaN wins for good
          best = v;
          at = (int32_t)k;
        }
      }
      s_val[tc][mi] = best;
      s_arg[tc][mi] = at;
    }
  }
  __syncthreads();
  {
    const int mi = threadIdx.x & (MAX_TM - 1);
    const int64_t m = m0 + mi;
    for (int ci = threadIdx.x / MAX_TM; ci < MAX_TC; ci += MAX_T / MAX_TM) {
      const int c = c0 + ci;
      if (c >= Cout || m >= M) continue;
      const int64_t o = (b * Cout + c) * M + m;
      out[o] = s_val[ci][mi];
      arg[o] = s_arg[ci][mi];
    }
  }
}

__global__ __launch_bounds__(MAX_T) void rows_max_bwd_k(const float* __restrict__ g, const int32_t* __restrict__ arg,
                                                        int64_t M, int64_t K, int Cout, int tiles_m, int tiles_c,
                                                        float* __restrict__ dY) {
  __shared__ float s_val[MAX_TC][MAX_PAD];
  __shared__ int32_t s_arg[MAX_TC][MAX_PAD];
  const int tile_c = blockIdx.x % tiles_c;
  const int64_t bt = blockIdx.x / tiles_c;
  const int64_t b = bt / tiles_m, m0 = (bt % tiles_m) * MAX_TM;
  const int c0 = tile_c * MAX_TC;
  {
    const int mi = threadIdx.x & (MAX_TM - 1);
    const int64_t m = m0 + mi;
    for (int ci = threadIdx.x / MAX_TM; ci < MAX_TC; ci += MAX_T / MAX_TM) {
      const int c = c0 + ci;
      if (c >= Cout || m >= M) continue;
      const int64_t o = (b * Cout + c) * M + m;
      s_val[ci][mi] = g[o];
      s_arg[ci][mi] = arg[o];
    }
  }
  __syncthreads();
  {
    const int tc = threadIdx.x & (MAX_TC - 1);
    const int c = c0 + tc;
    for (int mi = threadIdx.x / MAX_TC; mi < MAX_TM; mi += MAX_T / MAX_TC) {
      const int64_t m = m0 + mi;
      if (c >= Cout || m >= M) continue;
      const float v = s_val[tc][mi];
      const int64_t at = s_arg[tc][mi];
      float* y = dY + ((b * M + m) * K) * Cout + c;
      for (int64_t k = 0; k < K; ++k) y[k * Cout] = k == at ? v : 0.f;
    }
  }
}

int rows_sizes(const char* what, int B, int C, int64_t N, int64_t M, int K, int64_t* R) {
  MVK_REQUIRE(B >= 0 && C >= 0 && N >= 0 && M >= 0 && K >= 0, "%s: bad sizes B=%d C=%d N=%lld M=%lld K=%d", what, B, C,
              (long long)N, (long long)M, K);
  MVK_REQUIRE(M == 0 || K == 0 || ((int64_t)B * M < ROWS_LIMIT && (int64_t)B * M * K < ROWS_LIMIT),
              "%s: R = B*M*K = %d*%lld*%d must be below 2^31", what, B, (long long)M, K);
  MVK_REQUIRE((int64_t)B * N < ROWS_LIMIT, "%s: B*N must be below 2^31", what);
  *R = (int64_t)B * M * K;
  return 0;
}

int max_sizes(const char* what, int B, int64_t M, int K, int Cout, int64_t* blocks, int* tiles_m, int* tiles_c) {
  MVK_REQUIRE(B >= 0 && M >= 0 && K >= 1 && Cout >= 0, "%s: bad sizes B=%d M=%lld K=%d Cout=%d (K >= 1)", what, B,
              (long long)M, K, Cout);
  MVK_REQUIRE(M == 0 || ((int64_t)B * M < ROWS_LIMIT && (int64_t)B * M * K < ROWS_LIMIT),
              "%s: R = B*M*K = %d*%lld*%d must be below 2^31", what, B, (long long)M, K);
  const int64_t tm = cdiv64(M, MAX_TM), tc = cdiv64(Cout, MAX_TC);
  *blocks = (int64_t)B * tm * tc;
  MVK_REQUIRE(*blocks < ROWS_LIMIT, "%s: too many tiles", what);
  *tiles_m = (int)tm;
  *tiles_c = (int)tc;
  return 0;
}

}  // namespace

extern "C" int mvk_pn2_sa_rows_fwd(const float* xyz, const float* feature, const float* new_xyz, const int64_t* index,
                                   int B, int C, int use_xyz, int64_t N, int64_t M, int K, float* X, void* stream) {
  int64_t R;
  if (int rc = rows_sizes("pn2_sa_rows_fwd", B, C, N, M, K, &R)) return rc;
  if (!feature) {
    C = 0;
    use_xyz = 1;
  }
  MVK_REQUIRE(C > 0 || use_xyz, "pn2_sa_rows_fwd: rows without features and without coordinates");
  if (R == 0) return 0;
  MVK_REQUIRE(xyz && new_xyz && index && X, "pn2_sa_rows_fwd: null operand");
  const int groups = C >= 64 ? 8 : C >= 16 ? 4 : 1;                      // enough workgroups at small R, few index re-reads
  hipLaunchKernelGGL(sa_rows_fwd_k, dim3((unsigned)cdiv64(R, ROWS_T), groups), dim3(ROWS_T), 0, (hipStream_t)stream, xyz,
                     feature, new_xyz, index, C, use_xyz ? 1 : 0, N, M, (int64_t)K, R, X);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_sa_rows_bwd(const float* dX, const int64_t* index, int B, int C, int64_t N, int64_t M, int K,
                                   float* dfeature, void* stream) {
  int64_t R;
  if (int rc = rows_sizes("pn2_sa_rows_bwd", B, C, N, M, K, &R)) return rc;
  if (R == 0 || C == 0) return 0;
  MVK_REQUIRE(dX && index && dfeature, "pn2_sa_rows_bwd: null operand");
  const int64_t blocks = cdiv64((int64_t)C * R, ROWS_T);
  MVK_REQUIRE(blocks < ROWS_LIMIT, "pn2_sa_rows_bwd: too many elements");
  hipLaunchKernelGGL(sa_rows_bwd_k, dim3((unsigned)blocks), dim3(ROWS_T), 0, (hipStream_t)stream, dX, index, C, N,
                     M * (int64_t)K, R, dfeature);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_sa_rows_bwd_csr(const float* dX, const int32_t* row_start, const int32_t* entries, int B, int C,
                                       int64_t N, int64_t M, int K, float* dfeature, void* stream) {
  int64_t R;
  if (int rc = rows_sizes("pn2_sa_rows_bwd_csr", B, C, N, M, K, &R)) return rc;
  if ((int64_t)B * C * N == 0) return 0;
  MVK_REQUIRE(row_start && entries && dfeature && (R == 0 || dX), "pn2_sa_rows_bwd_csr: null operand");
  const int64_t nchunk = cdiv64(C, ROWS_CH), nkeyblk = cdiv64(N, ROWS_T);
  const int64_t blocks = (int64_t)B * nchunk * nkeyblk;
  MVK_REQUIRE(blocks < ROWS_LIMIT, "pn2_sa_rows_bwd_csr: too many elements");
  hipLaunchKernelGGL(sa_rows_bwd_csr_k, dim3((unsigned)blocks), dim3(ROWS_T), 0, (hipStream_t)stream, dX, row_start,
                     entries, C, N, M * (int64_t)K, R, (int)nchunk, (int)nkeyblk, dfeature);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_rows_max_fwd(const float* Y, int B, int64_t M, int K, int Cout, float* out, int32_t* arg,
                                    void* stream) {
  int64_t blocks;
  int tiles_m, tiles_c;
  if (int rc = max_sizes("pn2_rows_max_fwd", B, M, K, Cout, &blocks, &tiles_m, &tiles_c)) return rc;
  if (blocks == 0) return 0;
  MVK_REQUIRE(Y && out && arg, "pn2_rows_max_fwd: null operand");
  hipLaunchKernelGGL(rows_max_fwd_k, dim3((unsigned)blocks), dim3(MAX_T), 0, (hipStream_t)stream, Y, M, (int64_t)K, Cout,
                     tiles_m, tiles_c, out, arg);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_rows_max_bwd(const float* g, const int32_t* arg, int B, int64_t M, int K, int Cout, float* dY,
                                    void* stream) {
  int64_t blocks;
  int tiles_m, tiles_c;
  if (int rc = max_sizes("pn2_rows_max_bwd", B, M, K, Cout, &blocks, &tiles_m, &tiles_c)) return rc;
  if (blocks == 0) return 0;
  MVK_REQUIRE(g && arg && dY, "pn2_rows_max_bwd: null operand");
  hipLaunchKernelGGL(rows_max_bwd_k, dim3((unsigned)blocks), dim3(MAX_T), 0, (hipStream_t)stream, g, arg, M, (int64_t)K,
                     Cout, tiles_m, tiles_c, dY);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
