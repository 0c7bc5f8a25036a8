// PointNet++ / MVPNet in TRAINING mode on the library's GEMM and BatchNorm: the two ends of a shared
// MLP that the products and bn_lrelu do not cover, each with its backward -- for a SetAbstraction's ball-query group
// and for FeatureAggregation's 2D -> 3D hand-off over a whole batch. Both gather from a strided map (pn2_rows.h): the
// 2D encoder's output as it lies (NCHW or channels-last), or a point feature (B, C, N) as one image of N pixels per
// batch element. Compiled with -ffp-contract=off: every subtraction, product and addition below is one rounding.
//
//   rows_fwd_k<Tail>    the input rows of the shared MLP as the channel-major operand X [C (+tail), R], R = B*np*K,
//                       row r = (b*np + n)*K + k = [map(b*nv + p / hw, :, p % hw) | tail], p = index[b, n, k]. Lanes
//                       run along r: the index read and every store are coalesced, each gathered 4-byte read stays
//                       inside one channel plane (L2 resident), as in group_points_fwd_kernel and fa_gather_kernel.
//                       Channel groups in grid.y; group 0 also writes the tail:
//                         SaTail   xyz[b, :, p] - new_xyz[b, :, n] from channel-major coordinates, three rows
//                                  (QueryGrouper's order)
//                         FaTail   d = image_xyz[b, p] - points[b, :, n] from pixel-major image_xyz and
//                                  (d.x*d.x + d.y*d.y) + d.z*d.z, four rows (fa_relation)
//                       SetAbstraction always takes it; FeatureAggregation for a map whose pixels are contiguous
//                       inside a channel plane (NCHW) and for any other strides.
//   fa_rows_fwd_cl_k    FeatureAggregation's rows from a map whose CHANNELS are contiguous inside a pixel
//                       (channels-last): a workgroup owns 64 rows x 64 channels, reads each row's run of channels
//                       with lanes along the channels (256-byte segments), turns the tile in LDS (odd stride) and
//                       stores with lanes along r (256-byte segments of a row of X).
//   rows_bwd_k          dmap(b*nv + view, c, pix) += dX[c, r]: float atomics onto a zeroed map, one lane per (c, r)
//                       (the default mode).
//   fa_rows_bwd_cl_k    the same for a channels-last map through the 64 x 64 tile: every atomic wave-instruction adds
//                       onto the 256 contiguous bytes of one pixel instead of 64 pixels.
//                       The same sums in a fixed order (ops.set_deterministic) are ordered_bwd_k's, pn2_ordered.hip.
//   rows_reduce_k<Op>   Y [R, Cout] row-major (what bn_lrelu returns) -> out [B, Cout, M] over the K rows of a
//                       centroid. A workgroup owns TILE_M centroids x TILE_C channels: lanes along channels while
//                       reading (256-byte segments of a row), a padded LDS tile, lanes along M while storing
//                       (128-byte segments of a channel plane).
//                         RowsMax  the maximum and arg = the smallest k attaining it (strict >); the first NaN sticks
//                         RowsSum  acc = Y[first row], then acc = fl(acc + Y[row]) in ascending k; no arg, nor in LDS
//   rows_expand_k<Op>   g (and arg) [B, Cout, M] -> dY [R, Cout]: the same tile the other way round; every element
//                       of dY is written (Max: g at arg, +0 elsewhere; Sum: g in each of the K rows), no zero fill,
//                       no atomics.
// No kernel reads anything back; grids are fixed by the sizes: all of them are capturable.
#include "pn2_rows.h"

namespace {

constexpr int ROWS_T = 256;
constexpr int FA_CL_MIN = 8;        // fewer contiguous channels than this: the 64-channel-wide passes would idle
constexpr int FA_TR = 64;           // rows per tile of the channels-last kernels
constexpr int FA_TC = 64;           // channels per tile
constexpr int FA_PAD = FA_TR + 1;   // odd stride: lanes along channels and lanes along rows both hit distinct banks
constexpr int TILE_M = 32;          // centroids per tile of the reduction
constexpr int TILE_C = 64;          // channels per tile
constexpr int TILE_PAD = TILE_M + 1; // odd stride: a wave's ds_write (lanes along channels) hits 32 banks per half

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

// The rows that follow the C gathered channels of column e = (b, n, k), which selected key p (ok: p is inside the map).
struct SaTail {                     // xyz [B,3,N], new_xyz [B,3,M]: rows C .. C+2
  const float *xyz, *new_xyz;
  int64_t N, M;
  __device__ __forceinline__ void operator()(int64_t b, int64_t n, int64_t p, bool ok, int C, int64_t R, int64_t e,
                                             float* __restrict__ X) const {
    const float* q = xyz + b * 3 * N + (ok ? p : 0);
    const float* t = new_xyz + b * 3 * M + n;
#pragma unroll
    for (int d = 0; d < 3; ++d) X[(int64_t)(C + d) * R + e] = (ok ? q[d * N] : 0.f) - t[d * M];
  }
};
struct FaTail {                     // image_xyz [B,P,3], points [B,3,np]: rows C .. C+3
  const float *image_xyz, *points;
  int64_t P, np;
  __device__ __forceinline__ void operator()(int64_t b, int64_t n, int64_t p, bool ok, int C, int64_t R, int64_t e,
                                             float* __restrict__ X) const {
    fa_relation(image_xyz, points, b, n, p, ok, P, np, C, R, e, X);
  }
};

// grid (ceil(R / 256), channel groups): every group strides over the channels, group 0 also writes the tail
template <typename Tail>
__global__ __launch_bounds__(ROWS_T) void rows_fwd_k(const float* __restrict__ map, MapStrides s,
                                                     const int64_t* __restrict__ index, int C, int64_t nv, int64_t hw,
                                                     int64_t np, int64_t K, int64_t R, int use_tail, Tail tail,
                                                     float* __restrict__ X) {
  const int64_t e = (int64_t)blockIdx.x * ROWS_T + threadIdx.x;
  if (e >= R) return;
  const int64_t p = index[e];
  const int64_t bn = e / K, b = bn / np;
  const int64_t off = map_pixel(p, b, nv, hw, s);
  const bool ok = off >= 0;
  const float* f = map + (ok ? off : 0);
  for (int c = blockIdx.y; c < C; c += gridDim.y) X[(int64_t)c * R + e] = ok ? f[(int64_t)c * s.sc] : 0.f;
  if (use_tail && blockIdx.y == 0) tail(b, bn - b * np, p, ok, C, R, e, X);
}

// the first wave of a channels-last tile: the pixel offsets of the tile's 64 rows (-1: nothing to read, or no such row)
__device__ __forceinline__ void fa_tile_rows(const int64_t* __restrict__ index, int64_t r0, int64_t nv, int64_t hw,
                                             int64_t np, int64_t K, int64_t R, MapStrides s, int64_t* s_off) {
  const int64_t e = r0 + threadIdx.x;
  int64_t off = -1;
  if (e < R) off = map_pixel(index[e], e / K / np, nv, hw, s);
  s_off[threadIdx.x] = off;
}

// grid (ceil(R / 64), ceil(C / 64)); s.sc == 1
__global__ __launch_bounds__(ROWS_T) void fa_rows_fwd_cl_k(const float* __restrict__ map, MapStrides s,
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
    for (int ri = threadIdx.x / FA_TC; ri < FA_TR; ri += ROWS_T / FA_TC) {
      const int64_t off = s_off[ri];
      s_val[tc][ri] = (off >= 0 && c < C) ? map[off + c] : 0.f;
    }
  }
  __syncthreads();
  {
    const int ri = threadIdx.x & (FA_TR - 1);
    const int64_t e = r0 + ri;
    for (int ci = threadIdx.x / FA_TR; ci < FA_TC; ci += ROWS_T / FA_TR) {
      const int c = c0 + ci;
      if (c < C && e < R) X[(int64_t)c * R + e] = s_val[ci][ri];
    }
  }
}

// one lane per (channel, row); L = np*K rows per batch element
__global__ __launch_bounds__(ROWS_T) void rows_bwd_k(const float* __restrict__ dX, const int64_t* __restrict__ index,
                                                     int C, int64_t nv, int64_t hw, int64_t L, int64_t R,
                                                     float* __restrict__ dmap, MapStrides s) {
  const int64_t t = (int64_t)blockIdx.x * ROWS_T + threadIdx.x;
  if (t >= (int64_t)C * R) return;
  const int64_t c = t / R, e = t - c * R;
  const int64_t off = map_pixel(index[e], e / L, nv, hw, s);
  if (off >= 0) atomicAdd(dmap + off + c * s.sc, dX[t]);
}

// grid (ceil(R / 64), ceil(C / 64)); s.sc == 1
__global__ __launch_bounds__(ROWS_T) void fa_rows_bwd_cl_k(const float* __restrict__ dX,
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
    for (int ci = threadIdx.x / FA_TR; ci < FA_TC; ci += ROWS_T / FA_TR) {
      const int c = c0 + ci;
      s_val[ci][ri] = (c < C && e < R) ? dX[(int64_t)c * R + e] : 0.f;
    }
  }
  __syncthreads();
  {
    const int tc = threadIdx.x & (FA_TC - 1);
    const int c = c0 + tc;
    for (int ri = threadIdx.x / FA_TC; ri < FA_TR; ri += ROWS_T / FA_TC) {
      const int64_t off = s_off[ri];
      if (off >= 0 && c < C) atomicAdd(dmap + off + c, s_val[tc][ri]);
    }
  }
}

// What a tile does with the K rows of one (centroid, channel): y walks them with stride Cout.
struct RowsMax {
  static constexpr bool ARG = true;
  static __device__ __forceinline__ float reduce(const float* __restrict__ y, int64_t K, int Cout, int32_t* at) {
    float best = y[0];
    *at = 0;
    for (int64_t k = 1; k < K; ++k) {
      const float v = y[k * Cout];
      if (v > best || (v != v && best == best)) {          // strict: the smallest k; the first NaN wins for good
        best = v;
        *at = (int32_t)k;
      }
    }
    return best;
  }
  static __device__ __forceinline__ float expand(float v, int64_t at, int64_t k) { return k == at ? v : 0.f; }
};
struct RowsSum {
  static constexpr bool ARG = false;
  static __device__ __forceinline__ float reduce(const float* __restrict__ y, int64_t K, int Cout, int32_t*) {
    float acc = y[0];
    for (int64_t k = 1; k < K; ++k) acc = acc + y[k * Cout];
    return acc;
  }
  static __device__ __forceinline__ float expand(float v, int64_t, int64_t) { return v; }
};

template <bool ARG>
struct RowsTile {
  float val[TILE_C][TILE_PAD];
  int32_t arg[TILE_C][TILE_PAD];
};
template <>
struct RowsTile<false> {            // the sum carries no argument
  float val[TILE_C][TILE_PAD];
};

// blockIdx.x = (b * tiles_m + tile_m) * tiles_c + tile_c; arg is read and written for Op::ARG only
template <typename Op>
__global__ __launch_bounds__(ROWS_T) void rows_reduce_k(const float* __restrict__ Y, int64_t M, int64_t K, int Cout,
                                                        int tiles_m, int tiles_c, float* __restrict__ out,
                                                        int32_t* __restrict__ arg) {
  __shared__ RowsTile<Op::ARG> tile;
  const int tile_c = blockIdx.x % tiles_c;
  const int64_t bt = blockIdx.x / tiles_c;
  const int64_t b = bt / tiles_m, m0 = (bt % tiles_m) * TILE_M;
  const int c0 = tile_c * TILE_C;
  {
    const int tc = threadIdx.x & (TILE_C - 1);
    const int c = c0 + tc;
    for (int mi = threadIdx.x / TILE_C; mi < TILE_M; mi += ROWS_T / TILE_C) {
      const int64_t m = m0 + mi;
      if (c >= Cout || m >= M) continue;
      int32_t at = 0;
      tile.val[tc][mi] = Op::reduce(Y + ((b * M + m) * K) * Cout + c, K, Cout, &at);
      if constexpr (Op::ARG) tile.arg[tc][mi] = at;
    }
  }
  __syncthreads();
  {
    const int mi = threadIdx.x & (TILE_M - 1);
    const int64_t m = m0 + mi;
    for (int ci = threadIdx.x / TILE_M; ci < TILE_C; ci += ROWS_T / TILE_M) {
      const int c = c0 + ci;
      if (c >= Cout || m >= M) continue;
      const int64_t o = (b * Cout + c) * M + m;
      out[o] = tile.val[ci][mi];
      if constexpr (Op::ARG) arg[o] = tile.arg[ci][mi];
    }
  }
}

template <typename Op>
__global__ __launch_bounds__(ROWS_T) void rows_expand_k(const float* __restrict__ g, const int32_t* __restrict__ arg,
                                                        int64_t M, int64_t K, int Cout, int tiles_m, int tiles_c,
                                                        float* __restrict__ dY) {
  __shared__ RowsTile<Op::ARG> tile;
  const int tile_c = blockIdx.x % tiles_c;
  const int64_t bt = blockIdx.x / tiles_c;
  const int64_t b = bt / tiles_m, m0 = (bt % tiles_m) * TILE_M;
  const int c0 = tile_c * TILE_C;
  {
    const int mi = threadIdx.x & (TILE_M - 1);
    const int64_t m = m0 + mi;
    for (int ci = threadIdx.x / TILE_M; ci < TILE_C; ci += ROWS_T / TILE_M) {
      const int c = c0 + ci;
      if (c >= Cout || m >= M) continue;
      const int64_t o = (b * Cout + c) * M + m;
      tile.val[ci][mi] = g[o];
      if constexpr (Op::ARG) tile.arg[ci][mi] = arg[o];
    }
  }
  __syncthreads();
  {
    const int tc = threadIdx.x & (TILE_C - 1);
    const int c = c0 + tc;
    for (int mi = threadIdx.x / TILE_C; mi < TILE_M; mi += ROWS_T / TILE_C) {
      const int64_t m = m0 + mi;
      if (c >= Cout || m >= M) continue;
      const float v = tile.val[tc][mi];
      int64_t at = 0;
      if constexpr (Op::ARG) at = tile.arg[tc][mi];
      float* y = dY + ((b * M + m) * K) * Cout + c;
      for (int64_t k = 0; k < K; ++k) y[k * Cout] = Op::expand(v, at, k);
    }
  }
}

// the plane (lanes-along-rows) builder: one channel-group rule for both callers
template <typename Tail>
int launch_rows_fwd(const float* map, MapStrides s, const int64_t* index, int C, int64_t nv, int64_t hw, int64_t np,
                     int K, int64_t R, int use_tail, Tail tail, float* X, void* stream) {
  const int groups = C >= 64 ? 8 : C >= 16 ? 4 : 1;         // enough workgroups at small R, few index re-reads
  hipLaunchKernelGGL(rows_fwd_k<Tail>, dim3((unsigned)cdiv64(R, ROWS_T), groups), dim3(ROWS_T), 0, (hipStream_t)stream,
                     map, s, index, C, nv, hw, np, (int64_t)K, R, use_tail ? 1 : 0, tail, X);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

// the plane scatter
int launch_rows_bwd(const char* what, const float* dX, const int64_t* index, int C, int64_t nv, int64_t hw, int64_t L,
                    int64_t R, float* dmap, MapStrides s, void* stream) {
  const int64_t blocks = cdiv64((int64_t)C * R, ROWS_T);
  MVK_REQUIRE(blocks < ROWS_LIMIT, "%s: too many elements", what);
  hipLaunchKernelGGL(rows_bwd_k, dim3((unsigned)blocks), dim3(ROWS_T), 0, (hipStream_t)stream, dX, index, C, nv, hw, L,
                     R, dmap, s);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

// a pixel's channels are one contiguous run that is worth a 64-lane pass. FeatureAggregation's rule alone: a
// SetAbstraction asks for the plane kernels by name (with N == 1 its feature's channel stride is 1 as well).
bool channel_runs(MapStrides s, int C) { return s.sc == 1 && C >= FA_CL_MIN; }

int tile_sizes(const char* what, int B, int64_t M, int K, int Cout, int64_t* blocks, int* tiles_m, int* tiles_c) {
  MVK_REQUIRE(B >= 0 && M >= 0 && K >= 1 && Cout >= 0, "%s: bad sizes B=%d M=%lld K=%d Cout=%d (K >= 1)", what, B,
              (long long)M, K, Cout);
  MVK_REQUIRE(M == 0 || ((int64_t)B * M < ROWS_LIMIT && (int64_t)B * M * K < ROWS_LIMIT),
              "%s: R = B*M*K = %d*%lld*%d must be below 2^31", what, B, (long long)M, K);
  const int64_t tm = cdiv64(M, TILE_M), tc = cdiv64(Cout, TILE_C);
  *blocks = (int64_t)B * tm * tc;
  MVK_REQUIRE(*blocks < ROWS_LIMIT, "%s: too many tiles", what);
  *tiles_m = (int)tm;
  *tiles_c = (int)tc;
  return 0;
}

template <typename Op>
int rows_reduce_entry(const char* what, const float* Y, int B, int64_t M, int K, int Cout, float* out, int32_t* arg,
                      void* stream) {
  int64_t blocks;
  int tiles_m, tiles_c;
  if (int rc = tile_sizes(what, B, M, K, Cout, &blocks, &tiles_m, &tiles_c)) return rc;
  if (blocks == 0) return 0;
  MVK_REQUIRE(Y && out && (!Op::ARG || arg), "%s: null operand", what);
  hipLaunchKernelGGL(rows_reduce_k<Op>, dim3((unsigned)blocks), dim3(ROWS_T), 0, (hipStream_t)stream, Y, M, (int64_t)K,
                     Cout, tiles_m, tiles_c, out, arg);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename Op>
int rows_expand_entry(const char* what, const float* g, const int32_t* arg, int B, int64_t M, int K, int Cout,
                      float* dY, void* stream) {
  int64_t blocks;
  int tiles_m, tiles_c;
  if (int rc = tile_sizes(what, B, M, K, Cout, &blocks, &tiles_m, &tiles_c)) return rc;
  if (blocks == 0) return 0;
  MVK_REQUIRE(g && dY && (!Op::ARG || arg), "%s: null operand", what);
  hipLaunchKernelGGL(rows_expand_k<Op>, dim3((unsigned)blocks), dim3(ROWS_T), 0, (hipStream_t)stream, g, arg, M,
                     (int64_t)K, Cout, tiles_m, tiles_c, dY);
  MVK_CHECK_HIP(hipGetLastError());
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
  return launch_rows_fwd(feature, MapStrides{C * N, N, 1}, index, C, 1, N, M, K, R, use_xyz, SaTail{xyz, new_xyz, N, M},
                         X, stream);
}

extern "C" int mvk_pn2_sa_rows_bwd(const float* dX, const int64_t* index, int B, int C, int64_t N, int64_t M, int K,
                                   float* dfeature, void* stream) {
  int64_t R;
  if (int rc = rows_sizes("pn2_sa_rows_bwd", B, C, N, M, K, &R)) return rc;
  if (R == 0 || C == 0) return 0;
  MVK_REQUIRE(dX && index && dfeature, "pn2_sa_rows_bwd: null operand");
  return launch_rows_bwd("pn2_sa_rows_bwd", dX, index, C, 1, N, M * (int64_t)K, R, dfeature, MapStrides{C * N, N, 1},
                         stream);
}

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
  if (!channel_runs(s, C))
    return launch_rows_fwd(feature_2d, s, index, C, nv, HW, N, K, R, use_relation, FaTail{image_xyz, points, P, N}, X,
                           stream);
  hipLaunchKernelGGL(fa_rows_fwd_cl_k, dim3((unsigned)cdiv64(R, FA_TR), (unsigned)cdiv64(C, FA_TC)), dim3(ROWS_T), 0,
                     (hipStream_t)stream, feature_2d, s, image_xyz, points, index, C, use_relation ? 1 : 0, (int64_t)nv,
                     HW, N, (int64_t)K, R, X);
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
  if (!channel_runs(s, C))
    return launch_rows_bwd("pn2_fa_rows_bwd", dX, index, C, nv, HW, N * (int64_t)K, R, dfeature_2d, s, stream);
  hipLaunchKernelGGL(fa_rows_bwd_cl_k, dim3((unsigned)cdiv64(R, FA_TR), (unsigned)cdiv64(C, FA_TC)), dim3(ROWS_T), 0,
                     (hipStream_t)stream, dX, index, C, (int64_t)nv, HW, N, (int64_t)K, R, dfeature_2d, s);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_rows_max_fwd(const float* Y, int B, int64_t M, int K, int Cout, float* out, int32_t* arg,
                                    void* stream) {
  return rows_reduce_entry<RowsMax>("pn2_rows_max_fwd", Y, B, M, K, Cout, out, arg, stream);
}
extern "C" int mvk_pn2_rows_max_bwd(const float* g, const int32_t* arg, int B, int64_t M, int K, int Cout, float* dY,
                                    void* stream) {
  return rows_expand_entry<RowsMax>("pn2_rows_max_bwd", g, arg, B, M, K, Cout, dY, stream);
}
extern "C" int mvk_pn2_rows_sum_fwd(const float* Y, int B, int64_t M, int K, int Cout, float* out, void* stream) {
  return rows_reduce_entry<RowsSum>("pn2_rows_sum_fwd", Y, B, M, K, Cout, out, nullptr, stream);
}
extern "C" int mvk_pn2_rows_sum_bwd(const float* g, int B, int64_t M, int K, int Cout, float* dY, void* stream) {
  return rows_expand_entry<RowsSum>("pn2_rows_sum_bwd", g, nullptr, B, M, K, Cout, dY, stream);
}
