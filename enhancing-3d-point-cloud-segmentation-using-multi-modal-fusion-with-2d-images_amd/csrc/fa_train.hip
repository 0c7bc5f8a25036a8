// MVPNet's 2D -> 3D hand-off in TRAINING mode on the library's GEMM and BatchNorm: the two ends of
// FeatureAggregation's shared MLP for a whole batch, each with its backward. The map is the 2D encoder's output as it
// lies: element (image i, channel c, pixel q) at i * si + c * sc + q * sp (NCHW: C*hw, hw, 1; channels-last: C*hw, 1, C).
//
//   fa_rows_fwd_k       the input rows of the shared MLP as the channel-major operand X [C (+4), R], R = B*np*k, row
//                       r = (b*np + n)*k + j = [map(b*nv + p / hw, :, p % hw) | d | (d.x*d.x + d.y*d.y) + d.z*d.z],
//                       p = index[b, n, j], d = image_xyz[b, p] - points[b, :, n] (-ffp-contract=off: every operation is
//                       one rounding). Lanes along r, channel groups in grid.y: sa_rows_fwd_k on a strided map. Taken
//                       for a map whose pixels are contiguous inside a channel plane (NCHW) and for any other strides.
//   fa_rows_fwd_cl_k    the same rows from a map whose CHANNELS are contiguous inside a pixel (channels-last): a
//                       workgroup owns 64 rows x 64 channels, reads each row's run of channels with lanes along the
//                       channels (256-byte segments), turns the tile in LDS (odd stride) and stores with lanes along r
//                       (256-byte segments of a row of X): rows_max_fwd_k's tile the other way round.
//   fa_rows_bwd_k       dmap(b*nv + view, c, pix) += dX[c, r]: float atomics onto a zeroed map, one lane per (c, r).
//   fa_rows_bwd_cl_k    the same for a channels-last map through the 64 x 64 tile: every atomic wave-instruction adds
//                       onto the 256 contiguous bytes of one pixel instead of 64 pixels.
//   fa_rows_bwd_csr_k   the same sums in a fixed order over the transposed index (mvk_index_csr with n1 = nv*hw keys): a
//                       lane per pixel key, acc = fl(acc + g) over the key's positions in ascending order, every element
//                       of the map written (+0 without entries): sa_rows_bwd_csr_k's walk onto the map's own strides.
//   rows_sum_fwd_k      Y [R, Cout] row-major (what bn_lrelu returns) -> out [B, Cout, np]: acc = Y[first row], then
//                       acc = fl(acc + Y[row]) over the point's other k - 1 rows in ascending j. rows_max's tile: lanes
//                       along channels on the row side, a padded LDS tile, lanes along np on the plane side.
//   rows_sum_bwd_k      g [B, Cout, np] -> dY [R, Cout]: g in each of the point's k rows, every element written.
// No kernel reads anything back; grids are fixed by the sizes: all seven are capturable.
#include "common.h"

namespace {

constexpr int64_t FA_LIMIT = (int64_t)1 << 31;
constexpr int FA_T = 256;
constexpr int FA_CH = 8;            // channels per lane of fa_rows_bwd_csr_k
constexpr int FA_CL_MIN = 8;        // fewer contiguous channels than this: the 64-channel-wide passes would idle
constexpr int FA_TR = 64;           // rows per tile of the channels-last kernels
constexpr int FA_TC = 64;           // channels per tile
constexpr int FA_PAD = FA_TR + 1;   // odd stride: lanes along channels and lanes along rows both hit distinct banks
constexpr int SUM_TM = 32;          // points per tile of the sum (rows_max's tile)
constexpr int SUM_TC = 64;
constexpr int SUM_PAD = SUM_TM + 1;

struct MapStrides {
  int64_t si, sc, sp;
};

// where row e reads: the offset of its pixel's channel 0 in the map, or -1 for an index outside [0, nv*hw)
__device__ __forceinline__ int64_t fa_pixel(int64_t p, int64_t b, int64_t nv, int64_t hw, MapStrides s) {
  if (p < 0 || p >= nv * hw) return -1;
  const int64_t view = p / hw;
  return (b * nv + view) * s.si + (p - view * hw) * s.sp;
}

// rows C .. C+3 of column e
__device__ __forceinline__ void fa_relation(const float* __restrict__ image_xyz, const float* __restrict__ points,
                                            int64_t b, int64_t n, int64_t p, bool ok, int64_t P, int64_t np, int C,
                                            int64_t R, int64_t e, float* __restrict__ X) {
  const float* q = image_xyz + (b * P + (ok ? p : 0)) * 3;
  const float* t = points + b * 3 * np + n;
  const float dx = (ok ? q[0] : 0.f) - t[0];
  const float dy = (ok ? q[1] : 0.f) - t[np];
  const float dz = (ok ? q[2] : 0.f) - t[2 * np];
  X[(int64_t)C * R + e] = dx;
  X[(int64_t)(C + 1) * R + e] = dy;
  X[(int64_t)(C + 2) * R + e] = dz;
  X[(int64_t)(C + 3) * R + e] = (dx * dx + dy * dy) + dz * dz;
}

// grid (ceil(R / 256), channel groups): every group strides over the channels, group 0 also writes the relation rows
__global__ __launch_bounds__(FA_T) void fa_rows_fwd_k(const float* __restrict__ map, MapStrides s,
                                                      const float* __restrict__ image_xyz,
                                                      const float* __restrict__ points,
                                                      const int64_t* __restrict__ index, int C, int use_relation,
                                                      int64_t nv, int64_t hw, int64_t np, int64_t K, int64_t R,
                                                      float* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * FA_T + threadIdx.x;
  if (e >= R) return;
  const int64_t p = index[e];
  const int64_t bn = e / K, b = bn / np;
  const int64_t off = fa_pixel(p, b, nv, hw, s);
  const bool ok = off >= 0;
  const float* f = map + (ok ? off : 0);
  for (int c = blockIdx.y; c < C; c += gridDim.y) X[(int64_t)c * R + e] = ok ? f[(int64_t)c * s.sc] : 0.f;
  if (use_relation && blockIdx.y == 0) fa_relation(image_xyz, points, b, bn - b * np, p, ok, nv * hw, np, C, R, e, X);
}

// the first wave of a channels-last tile: the pixel offsets of the tile's 64 rows (-1: nothing to read, or no such row)
__device__ __forceinline__ void fa_tile_rows(const int64_t* __restrict__ index, int64_t r0, int64_t nv, int64_t hw,
                                             int64_t np, int64_t K, int64_t R, MapStrides s, int64_t* s_off) {
  const int64_t e = r0 + threadIdx.x;
  int64_t off = -1;
  if (e < R) off = fa_pixel(index[e], e / K / np, nv, hw, s);
  s_off[threadIdx.x] = off;
}

// grid (ceil(R / 64), ceil(C / 64)); s.sc == 1
__global__ __launch_bounds__(FA_T) void fa_rows_fwd_cl_k(const float* __restrict__ map, MapStrides s,
                                                         const float* __restrict__ image_xyz,
                                                         const float* __restrict__ points,
                                                         const int64_t* __restrict__ index, int C, int use_relation,
                                                         int64_t nv, int64_t hw, int64_t np, int64_t K, int64_t R,
                                                         float* __restrict__ X) {
  __shared__ float s_val[FA_TC][FA_PAD];
  __shared__ int64_t s_off[FA_TR];
  const int64_t r0 = (int64_t)blockIdx.x * FA_TR;
  const int c0 = blockIdx.y * FA_TC;
  if (threadIdx.x < FA_TR) {
    fa_tile_rows(index, r0, nv, hw, np, K, R, s, s_off);
    const int64_t e = r0 + threadIdx.x;
    if (use_relation && blockIdx.y == 0 && e < R) {
      const int64_t bn = e / K, b = bn / np;
      fa_relation(image_xyz, points, b, bn - b * np, index[e], s_off[threadIdx.x] >= 0, nv * hw, np, C, R, e, X);
    }
  }
  __syncthreads();
  {
    const int tc = threadIdx.x & (FA_TC - 1);
    const int c = c0 + tc;
    for (int ri = threadIdx.x / FA_TC; ri < FA_TR; ri += FA_T / FA_TC) {
      const int64_t off = s_off[ri];
      s_val[tc][ri] = (off >= 0 && c < C) ? map[off + c] : 0.f;
    }
  }
  __syncthreads();
  {
    const int ri = threadIdx.x & (FA_TR - 1);
    const int64_t e = r0 + ri;
    for (int ci = threadIdx.x / FA_TR; ci < FA_TC; ci += FA_T / FA_TR) {
      const int c = c0 + ci;
      if (c < C && e < R) X[(int64_t)c * R + e] = s_val[ci][ri];
    }
  }
}

// one lane per (channel, row)
__global__ __launch_bounds__(FA_T) void fa_rows_bwd_k(const float* __restrict__ dX, const int64_t* __restrict__ index,
                                                      int C, int64_t nv, int64_t hw, int64_t L, int64_t R,
                                                      float* __restrict__ dmap, MapStrides s) {
  const int64_t t = (int64_t)blockIdx.x * FA_T + threadIdx.x;
  if (t >= (int64_t)C * R) return;
  const int64_t c = t / R, e = t - c * R;
  const int64_t off = fa_pixel(index[e], e / L, nv, hw, s);
  if (off >= 0) atomicAdd(dmap + off + c * s.sc, dX[t]);
}

// grid (ceil(R / 64), ceil(C / 64)); s.sc == 1
__global__ __launch_bounds__(FA_T) void fa_rows_bwd_cl_k(const float* __restrict__ dX,
                                                         const int64_t* __restrict__ index, int C, int64_t nv,
                                                         int64_t hw, int64_t np, int64_t K, int64_t R,
                                                         float* __restrict__ dmap, MapStrides s) {
  __shared__ float s_val[FA_TC][FA_PAD];
  __shared__ int64_t s_off[FA_TR];
  const int64_t r0 = (int64_t)blockIdx.x * FA_TR;
  const int c0 = blockIdx.y * FA_TC;
  if (threadIdx.x < FA_TR) fa_tile_rows(index, r0, nv, hw, np, K, R, s, s_off);
  {
    const int ri = threadIdx.x & (FA_TR - 1);
    const int64_t e = r0 + ri;
    for (int ci = threadIdx.x / FA_TR; ci < FA_TC; ci += FA_T / FA_TR) {
      const int c = c0 + ci;
      s_val[ci][ri] = (c < C && e < R) ? dX[(int64_t)c * R + e] : 0.f;
    }
  }
  __syncthreads();
  {
    const int tc = threadIdx.x & (FA_TC - 1);
    const int c = c0 + tc;
    for (int ri = threadIdx.x / FA_TC; ri < FA_TR; ri += FA_T / FA_TC) {
      const int64_t off = s_off[ri];
      if (off >= 0 && c < C) atomicAdd(dmap + off + c, s_val[tc][ri]);
    }
  }
}

// one workgroup = 256 pixel keys x FA_CH channels of one batch element (sa_rows_bwd_csr_k, pn2_train.hip)
__global__ __launch_bounds__(FA_T) void fa_rows_bwd_csr_k(const float* __restrict__ dX,
                                                          const int32_t* __restrict__ row_start,
                                                          const int32_t* __restrict__ entries, int C, int64_t nv,
                                                          int64_t hw, int64_t L, int64_t R, int nchunk, int nkeyblk,
                                                          float* __restrict__ dmap, MapStrides s) {
  const int kb = blockIdx.x % nkeyblk;
  const int bc = blockIdx.x / nkeyblk;
  const int chunk = bc % nchunk;
  const int64_t b = bc / nchunk;
  const int64_t P = nv * hw;
  const int64_t j = (int64_t)kb * FA_T + threadIdx.x;
  if (j >= P) return;
  const int c0 = chunk * FA_CH;
  const float* gp[FA_CH];
#pragma unroll
  for (int u = 0; u < FA_CH; ++u) {
    const int c = c0 + u < C ? c0 + u : C - 1;                           // a chunk's surplus lanes re-read the last channel
    gp[u] = dX + (int64_t)c * R + b * L;
  }
  float acc[FA_CH];
#pragma unroll
  for (int u = 0; u < FA_CH; ++u) acc[u] = 0.f;
  int64_t beg = row_start[b * P + j], end = row_start[b * P + j + 1];
  if (beg < 0) beg = 0;
  if (end > R) end = R;
  for (int64_t i = beg; i < end; ++i) {
    const int64_t p = entries[i];
    if (p < 0 || p >= L) continue;
#pragma unroll
    for (int u = 0; u < FA_CH; ++u) acc[u] = acc[u] + gp[u][p];
  }
  float* out = dmap + fa_pixel(j, b, nv, hw, s);
#pragma unroll
  for (int u = 0; u < FA_CH; ++u)
    if (c0 + u < C) out[(int64_t)(c0 + u) * s.sc] = acc[u];
}

// blockIdx.x = (b * tiles_m + tile_m) * tiles_c + tile_c
__global__ __launch_bounds__(FA_T) void rows_sum_fwd_k(const float* __restrict__ Y, int64_t M, int64_t K, int Cout,
                                                       int tiles_m, int tiles_c, float* __restrict__ out) {
  __shared__ float s_val[SUM_TC][SUM_PAD];
  const int tile_c = blockIdx.x % tiles_c;
  const int64_t bt = blockIdx.x / tiles_c;
  const int64_t b = bt / tiles_m, m0 = (bt % tiles_m) * SUM_TM;
  const int c0 = tile_c * SUM_TC;
  {
    const int tc = threadIdx.x & (SUM_TC - 1);
    const int c = c0 + tc;
    for (int mi = threadIdx.x / SUM_TC; mi < SUM_TM; mi += FA_T / SUM_TC) {
      const int64_t m = m0 + mi;
      if (c >= Cout || m >= M) continue;
      const float* y = Y + ((b * M + m) * K) * Cout + c;
      float acc = y[0];
      for (int64_t k = 1; k < K; ++k) acc = acc + y[k * Cout];
      s_val[tc][mi] = acc;
    }
  }
  __syncthreads();
  {
    const int mi = threadIdx.x & (SUM_TM - 1);
    const int64_t m = m0 + mi;
    for (int ci = threadIdx.x / SUM_TM; ci < SUM_TC; ci += FA_T / SUM_TM) {
      const int c = c0 + ci;
      if (c >= Cout || m >= M) continue;
      out[(b * Cout + c) * M + m] = s_val[ci][mi];
    }
  }
}

__global__ __launch_bounds__(FA_T) void rows_sum_bwd_k(const float* __restrict__ g, int64_t M, int64_t K, int Cout,
                                                       int tiles_m, int tiles_c, float* __restrict__ dY) {
  __shared__ float s_val[SUM_TC][SUM_PAD];
  const int tile_c = blockIdx.x % tiles_c;
  const int64_t bt = blockIdx.x / tiles_c;
  const int64_t b = bt / tiles_m, m0 = (bt % tiles_m) * SUM_TM;
  const int c0 = tile_c * SUM_TC;
  {
    const int mi = threadIdx.x & (SUM_TM - 1);
    const int64_t m = m0 + mi;
    for (int ci = threadIdx.x / SUM_TM; ci < SUM_TC; ci += FA_T / SUM_TM) {
      const int c = c0 + ci;
      if (c >= Cout || m >= M) continue;
      s_val[ci][mi] = g[(b * Cout + c) * M + m];
    }
  }
  __syncthreads();
  {
    const int tc = threadIdx.x & (SUM_TC - 1);
    const int c = c0 + tc;
    for (int mi = threadIdx.x / SUM_TC; mi < SUM_TM; mi += FA_T / SUM_TC) {
      const int64_t m = m0 + mi;
      if (c >= Cout || m >= M) continue;
      const float v = s_val[tc][mi];
      float* y = dY + ((b * M + m) * K) * Cout + c;
      for (int64_t k = 0; k < K; ++k) y[k * Cout] = v;
    }
  }
}

int fa_sizes(const char* what, int B, int nv, int C, int64_t hw, int64_t np, int K, MapStrides s, int64_t* R,
             int64_t* P) {
  MVK_REQUIRE(B >= 0 && nv >= 0 && C >= 0 && hw >= 0 && np >= 0 && K >= 0,
              "%s: bad sizes B=%d nv=%d C=%d hw=%lld np=%lld k=%d", what, B, nv, C, (long long)hw, (long long)np, K);
  MVK_REQUIRE(s.si >= 0 && s.sc >= 0 && s.sp >= 0, "%s: negative map stride", what);
  MVK_REQUIRE(np == 0 || K == 0 || ((int64_t)B * np < FA_LIMIT && (int64_t)B * np * K < FA_LIMIT),
              "%s: R = B*np*k = %d*%lld*%d must be below 2^31", what, B, (long long)np, K);
  MVK_REQUIRE(hw < FA_LIMIT && (int64_t)nv * hw < FA_LIMIT && (int64_t)B * nv * hw < FA_LIMIT,
              "%s: B*nv*hw = %d*%d*%lld must be below 2^31", what, B, nv, (long long)hw);
  *R = (int64_t)B * np * K;
  *P = (int64_t)nv * hw;
  return 0;
}

int sum_sizes(const char* what, int B, int64_t M, int K, int Cout, int64_t* blocks, int* tiles_m, int* tiles_c) {
  MVK_REQUIRE(B >= 0 && M >= 0 && K >= 1 && Cout >= 0, "%s: bad sizes B=%d M=%lld K=%d Cout=%d (K >= 1)", what, B,
              (long long)M, K, Cout);
  MVK_REQUIRE(M == 0 || ((int64_t)B * M < FA_LIMIT && (int64_t)B * M * K < FA_LIMIT),
              "%s: R = B*M*K = %d*%lld*%d must be below 2^31", what, B, (long long)M, K);
  const int64_t tm = cdiv64(M, SUM_TM), tc = cdiv64(Cout, SUM_TC);
  *blocks = (int64_t)B * tm * tc;
  MVK_REQUIRE(*blocks < FA_LIMIT, "%s: too many tiles", what);
  *tiles_m = (int)tm;
  *tiles_c = (int)tc;
  return 0;
}

// a pixel's channels are one contiguous run that is worth a 64-lane pass
bool channel_runs(MapStrides s, int C) { return s.sc == 1 && C >= FA_CL_MIN; }

}  // namespace

extern "C" int mvk_pn2_fa_rows_fwd(const float* feature_2d, int64_t stride_image, int64_t stride_channel,
                                   int64_t stride_pixel, const float* image_xyz, const float* points,
                                   const int64_t* index, int B, int nv, int C, int64_t HW, int64_t N, int K,
                                   int use_relation, float* X, void* stream) {
  const MapStrides s{stride_image, stride_channel, stride_pixel};
  int64_t R, P;
  if (int rc = fa_sizes("pn2_fa_rows_fwd", B, nv, C, HW, N, K, s, &R, &P)) return rc;
  MVK_REQUIRE(C > 0 || use_relation, "pn2_fa_rows_fwd: rows without features and without relation");
  if (R == 0) return 0;
  MVK_REQUIRE(index && X && (C == 0 || feature_2d) && (!use_relation || (image_xyz && points)),
              "pn2_fa_rows_fwd: null operand");
  if (channel_runs(s, C)) {
    hipLaunchKernelGGL(fa_rows_fwd_cl_k, dim3((unsigned)cdiv64(R, FA_TR), (unsigned)cdiv64(C, FA_TC)), dim3(FA_T), 0,
                       (hipStream_t)stream, feature_2d, s, image_xyz, points, index, C, use_relation ? 1 : 0,
                       (int64_t)nv, HW, N, (int64_t)K, R, X);
  } else {
    const int groups = C >= 64 ? 8 : C >= 16 ? 4 : 1;                    // sa_rows_fwd_k's rule
    hipLaunchKernelGGL(fa_rows_fwd_k, dim3((unsigned)cdiv64(R, FA_T), groups), dim3(FA_T), 0, (hipStream_t)stream,
                       feature_2d, s, image_xyz, points, index, C, use_relation ? 1 : 0, (int64_t)nv, HW, N, (int64_t)K,
                       R, X);
  }
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_fa_rows_bwd(const float* dX, const int64_t* index, int B, int nv, int C, int64_t HW, int64_t N,
                                   int K, float* dfeature_2d, int64_t stride_image, int64_t stride_channel,
                                   int64_t stride_pixel, void* stream) {
  const MapStrides s{stride_image, stride_channel, stride_pixel};
  int64_t R, P;
  if (int rc = fa_sizes("pn2_fa_rows_bwd", B, nv, C, HW, N, K, s, &R, &P)) return rc;
  if (R == 0 || C == 0 || P == 0) return 0;
  MVK_REQUIRE(dX && index && dfeature_2d, "pn2_fa_rows_bwd: null operand");
  if (channel_runs(s, C)) {
    hipLaunchKernelGGL(fa_rows_bwd_cl_k, dim3((unsigned)cdiv64(R, FA_TR), (unsigned)cdiv64(C, FA_TC)), dim3(FA_T), 0,
                       (hipStream_t)stream, dX, index, C, (int64_t)nv, HW, N, (int64_t)K, R, dfeature_2d, s);
  } else {
    const int64_t blocks = cdiv64((int64_t)C * R, FA_T);
    MVK_REQUIRE(blocks < FA_LIMIT, "pn2_fa_rows_bwd: too many elements");
    hipLaunchKernelGGL(fa_rows_bwd_k, dim3((unsigned)blocks), dim3(FA_T), 0, (hipStream_t)stream, dX, index, C,
                       (int64_t)nv, HW, N * (int64_t)K, R, dfeature_2d, s);
  }
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_fa_rows_bwd_csr(const float* dX, const int32_t* row_start, const int32_t* entries, int B, int nv,
                                       int C, int64_t HW, int64_t N, int K, float* dfeature_2d, int64_t stride_image,
                                       int64_t stride_channel, int64_t stride_pixel, void* stream) {
  const MapStrides s{stride_image, stride_channel, stride_pixel};
  int64_t R, P;
  if (int rc = fa_sizes("pn2_fa_rows_bwd_csr", B, nv, C, HW, N, K, s, &R, &P)) return rc;
  if ((int64_t)B * C * P == 0) return 0;
  MVK_REQUIRE(row_start && entries && dfeature_2d && (R == 0 || dX), "pn2_fa_rows_bwd_csr: null operand");
  const int64_t nchunk = cdiv64(C, FA_CH), nkeyblk = cdiv64(P, FA_T);
  const int64_t blocks = (int64_t)B * nchunk * nkeyblk;
  MVK_REQUIRE(blocks < FA_LIMIT, "pn2_fa_rows_bwd_csr: too many elements");
  hipLaunchKernelGGL(fa_rows_bwd_csr_k, dim3((unsigned)blocks), dim3(FA_T), 0, (hipStream_t)stream, dX, row_start,
                     entries, C, (int64_t)nv, HW, N * (int64_t)K, R, (int)nchunk, (int)nkeyblk, dfeature_2d, s);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_rows_sum_fwd(const float* Y, int B, int64_t M, int K, int Cout, float* out, void* stream) {
  int64_t blocks;
  int tiles_m, tiles_c;
  if (int rc = sum_sizes("pn2_rows_sum_fwd", B, M, K, Cout, &blocks, &tiles_m, &tiles_c)) return rc;
  if (blocks == 0) return 0;
  MVK_REQUIRE(Y && out, "pn2_rows_sum_fwd: null operand");
  hipLaunchKernelGGL(rows_sum_fwd_k, dim3((unsigned)blocks), dim3(FA_T), 0, (hipStream_t)stream, Y, M, (int64_t)K, Cout,
                     tiles_m, tiles_c, out);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_rows_sum_bwd(const float* g, int B, int64_t M, int K, int Cout, float* dY, void* stream) {
  int64_t blocks;
  int tiles_m, tiles_c;
  if (int rc = sum_sizes("pn2_rows_sum_bwd", B, M, K, Cout, &blocks, &tiles_m, &tiles_c)) return rc;
  if (blocks == 0) return 0;
  MVK_REQUIRE(g && dY, "pn2_rows_sum_bwd: null operand");
  hipLaunchKernelGGL(rows_sum_bwd_k, dim3((unsigned)blocks), dim3(FA_T), 0, (hipStream_t)stream, g, M, (int64_t)K, Cout,
                     tiles_m, tiles_c, dY);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
