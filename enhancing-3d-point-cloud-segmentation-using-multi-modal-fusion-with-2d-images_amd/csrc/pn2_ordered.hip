// The two PointNet++ backwards that scatter (feature_interpolate, group_points) as per-key GATHERS over the transposed
// index: every sum in a fixed order (ascending position), no float atomics, every output element written. The atomic
// forms stay where they are (interp_bwd_k in pn2.hip, group_points_bwd_kernel in fusion.hip) and stay the default; these
// run when ops.set_deterministic(True) was on in the forward. Compiled with -ffp-contract=off: a product and the
// addition that follows it are two roundings, which is what the NumPy oracle (tests/pn2_ordered_ref.py) computes.
//
// Both ops select keys in [0, N1) through an int64 index (B, N2, K) (K = 3 for the interpolation). Per batch element the
// index is a flat list of L = N2 * K positions p = n * K + k.
//
// mvk_index_csr: the transposed index as a CSR -- row (b, j) = the positions p with index[b, p] == j, ascending.
//   csr_zero_k         row_start[0 .. B*N1] and the caller's cursor words <- 0
//   csr_count_k        one lane per position: atomicAdd(row_start[b*N1 + j], 1) (integer: the count has no order);
//                      a position outside [0, N1) is in no row and raises the status word
//   csr_block_sums_k   \
//   csr_scan_sums_k     > exclusive prefix of the B*N1 + 1 counts in place, 1024 per workgroup (blockscan.h / compact.h)
//   csr_scan_apply_k   /
//   csr_fill_k         one lane per position: slot = atomicAdd(cursor[row], 1), entries[row_start[row] + slot] = p
//                      (the slot is the order of arrival: the row holds the right SET in some order)
//   csr_sort_k         four rows per workgroup. A row of up to CSR_WAVE_ROW entries is ranked by counting by one wave
//                      (the positions of a row are distinct) out of LDS. A longer row is not sorted at all: the workgroup
//                      reads index[b, 0 .. L) again and compacts the positions that hold j, in order (ballot + prefix
//                      popcount, 256 positions per round). That is O(L) for a row of any length, and a batch element has at
//                      most L / CSR_WAVE_ROW such rows.
// Seven launches, each with a grid fixed by (B, L, N1); nothing is read back.
//
// ordered_bwd_k: a lane per key j (consecutive lanes, consecutive keys: coalesced stores), CH channels per lane in
// registers while it walks its row once; the loads of grad_out are scattered inside rows of 4 * N2 bytes that stay in L2.
// A row's sum is sequential by contract, so a long row is one lane's loop (correct for any length, slow for a
// degenerate index where one key owns everything). It is the library's only per-key walk: the feature gradients of the
// training-mode row builders (pn2_rows.hip: a SetAbstraction's group rows, FeatureAggregation's rows onto the 2D
// encoder's strided map) are two more entries on it, at the end of this file.
#include "blockscan.h"
#include "compact.h"
#include "pn2_rows.h"

namespace {

constexpr int CSR_T = 256;
constexpr int CSR_ROWS = CSR_T / 64;                 // rows per workgroup of csr_sort_k: one per wave
constexpr int CSR_WAVE_ROW = 512;                    // longest row that a wave ranks out of LDS
constexpr int64_t CSR_LIMIT = (int64_t)1 << 31;

__global__ __launch_bounds__(CSR_T) void csr_zero_k(int32_t* __restrict__ row_start, int64_t n_rows,
                                                    int32_t* __restrict__ cursor, int64_t n_cursor) {
  const int64_t step = (int64_t)gridDim.x * CSR_T;
  for (int64_t i = (int64_t)blockIdx.x * CSR_T + threadIdx.x; i < n_rows; i += step) row_start[i] = 0;
  for (int64_t i = (int64_t)blockIdx.x * CSR_T + threadIdx.x; i < n_cursor; i += step) cursor[i] = 0;
}

__global__ __launch_bounds__(CSR_T) void csr_count_k(const int64_t* __restrict__ index, int64_t total, int64_t L,
                                                     int64_t N1, int32_t* __restrict__ count,
                                                     int32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * CSR_T + threadIdx.x;
  if (e >= total) return;
  const int64_t j = index[e];
  if (j >= 0 && j < N1)
    atomicAdd(count + (e / L) * N1 + j, 1);
  else if (status)
    *status = 1;
}

__global__ __launch_bounds__(TPB) void csr_block_sums_k(const int32_t* __restrict__ count, int64_t n,
                                                        int32_t* __restrict__ block_sums) {
  __shared__ int sh[TPB / 64 + 1];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int total;
  block_exclusive_scan(i < n ? count[i] : 0, &total, sh);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(COMPACT_T) void csr_scan_sums_k(int32_t* __restrict__ block_sums, int nblk) {
  __shared__ int carry;
  __shared__ int ws[COMPACT_WAVES];
  compact_scan_counts(block_sums, nblk, &carry, ws);
}

__global__ __launch_bounds__(TPB) void csr_scan_apply_k(int32_t* __restrict__ count, int64_t n,
                                                        const int32_t* __restrict__ block_sums) {
  __shared__ int sh[TPB / 64 + 1];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int total;
  const int x = block_exclusive_scan(i < n ? count[i] : 0, &total, sh);
  if (i < n) count[i] = x + block_sums[blockIdx.x];
}

__global__ __launch_bounds__(CSR_T) void csr_fill_k(const int64_t* __restrict__ index, int64_t total, int64_t L,
                                                    int64_t N1, const int32_t* __restrict__ row_start,
                                                    int32_t* __restrict__ cursor, int32_t* __restrict__ entries) {
  const int64_t e = (int64_t)blockIdx.x * CSR_T + threadIdx.x;
  if (e >= total) return;
  const int64_t j = index[e];
  if (j < 0 || j >= N1) return;
  const int64_t r = (e / L) * N1 + j;
  const int64_t dst = (int64_t)row_start[r] + atomicAdd(cursor + r, 1);
  if (dst >= 0 && dst < total) entries[dst] = (int32_t)(e % L);      // (always, while nobody rewrites the index under us)
}

__global__ __launch_bounds__(CSR_T) void csr_sort_k(const int64_t* __restrict__ index, int64_t R, int64_t L, int64_t N1,
                                                    int64_t total, const int32_t* __restrict__ row_start,
                                                    int32_t* __restrict__ entries) {
  __shared__ int32_t buf[CSR_ROWS][CSR_WAVE_ROW];
  __shared__ int wave_hits[CSR_ROWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * CSR_ROWS;
  {
    const int64_t r = r0 + wv;
    int64_t beg = 0, len = 0;
    if (r < R) {
      beg = row_start[r];
      len = (int64_t)row_start[r + 1] - beg;
      if (beg < 0 || len < 0 || beg + len > total || len > CSR_WAVE_ROW) len = 0;     // long rows: below
    }
    for (int i = lane; i < len; i += 64) buf[wv][i] = entries[beg + i];
    __syncthreads();
    for (int i = lane; i < len; i += 64) {
      const int32_t v = buf[wv][i];
      int rank = 0;
      for (int t = 0; t < len; ++t) rank += buf[wv][t] < v ? 1 : 0;      // broadcast reads; the positions are distinct
      entries[beg + rank] = v;
    }
  }
  for (int q = 0; q < CSR_ROWS; ++q) {                                    // every branch below is workgroup-uniform
    const int64_t r = r0 + q;
    if (r >= R) break;
    const int64_t beg = row_start[r], len = (int64_t)row_start[r + 1] - beg;
    if (len <= CSR_WAVE_ROW || beg < 0 || beg + len > total) continue;
    const int64_t j = r % N1;
    const int64_t* ix = index + (r / N1) * L;
    int64_t done = 0;
    for (int64_t base = 0; base < L; base += CSR_T) {
      const int64_t p = base + threadIdx.x;
      const bool hit = p < L && ix[p] == j;
      const unsigned long long m = __ballot(hit);
      if (lane == 0) wave_hits[wv] = __popcll(m);
      __syncthreads();
      int64_t off = done;
      int all = 0;
      for (int k = 0; k < CSR_ROWS; ++k) {
        off += k < wv ? wave_hits[k] : 0;
        all += wave_hits[k];
      }
      off += compact_lane_rank(m);
      if (hit && off < len) entries[beg + off] = (int32_t)p;
      done += all;
      __syncthreads();
    }
  }
}

// out(b, c, j) = the ordered sum over row (b, j), the only per-key walk of the library. The gradient g is a base pointer
// with a channel stride gc and a batch stride gb: (B, C, G) is (G, C*G), a channel-major operand [C, B*L] is (B*L, L).
// INTERP: entry p reads g[.., p / 3] * w[b, p]; otherwise entry p reads g[.., p]. The result goes onto a map of nv images
// of hw keys per batch element with strides s (pn2_rows.h): a plain (B, C, N1) gradient is nv = 1, hw = N1,
// (C*N1, N1, 1). One workgroup = 256 keys x CH channels of one batch element.
template <typename T, bool INTERP, int CH>
__global__ __launch_bounds__(256) void ordered_bwd_k(const T* __restrict__ g, int64_t gc, int64_t gb,
                                                     const T* __restrict__ w, const int32_t* __restrict__ row_start,
                                                     const int32_t* __restrict__ entries, int C, int64_t nv, int64_t hw,
                                                     int64_t L, int64_t total, int nchunk, int nkeyblk,
                                                     T* __restrict__ out, MapStrides s) {
  const int kb = blockIdx.x % nkeyblk;
  const int bc = blockIdx.x / nkeyblk;
  const int chunk = bc % nchunk;
  const int64_t b = bc / nchunk;
  const int64_t N1 = nv * hw;
  const int64_t j = (int64_t)kb * 256 + threadIdx.x;
  if (j >= N1) return;
  const int c0 = chunk * CH;
  const T* gp[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    const int c = c0 + u < C ? c0 + u : C - 1;                           // a chunk's surplus lanes re-read the last channel
    gp[u] = g + c * gc + b * gb;
  }
  T acc[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) acc[u] = (T)0;
  int64_t beg = row_start[b * N1 + j], end = row_start[b * N1 + j + 1];
  if (beg < 0) beg = 0;
  if (end > total) end = total;
  const T* wb = INTERP ? w + b * L : nullptr;
  for (int64_t i = beg; i < end; ++i) {
    const int64_t p = entries[i];
    if (p < 0 || p >= L) continue;
    const int64_t n = INTERP ? p / 3 : p;
    if (INTERP) {
      // the gathered values first, the weight last: with the weight's load in front the same instructions come out in
      // a schedule that measured 2 % slower (profiles/rows_refactor_bench.txt)
      T v[CH];
#pragma unroll
      for (int u = 0; u < CH; ++u) v[u] = gp[u][n];
      const T wk = wb[p];
#pragma unroll
      for (int u = 0; u < CH; ++u) acc[u] = acc[u] + v[u] * wk;
    } else {
#pragma unroll
      for (int u = 0; u < CH; ++u) acc[u] = acc[u] + gp[u][n];
    }
  }
  T* o = out + map_offset(j, b, nv, hw, s);
#pragma unroll
  for (int u = 0; u < CH; ++u)
    if (c0 + u < C) o[(c0 + u) * s.sc] = acc[u];
}

inline int64_t csr_scan_blocks(int64_t R) { return cdiv64(R + 1, TPB); }

// what every ordered backward does once its own size refusals have passed: L positions per batch element, the keys of
// the map (nv, hw, s)
template <typename T, bool INTERP>
int ordered_bwd_entry(const char* what, const T* g, int64_t gc, int64_t gb, const T* w, const int32_t* row_start,
                      const int32_t* entries, int B, int C, int64_t nv, int64_t hw, int64_t L, T* out, MapStrides s,
                      void* stream) {
  constexpr int CH = 8;
  const int64_t N1 = nv * hw;
  if ((int64_t)B * C * N1 == 0) return 0;
  MVK_REQUIRE(row_start && entries && out && (L == 0 || (g && (!INTERP || w))), "%s: null operand", what);
  const int64_t nchunk = cdiv64(C, CH), nkeyblk = cdiv64(N1, 256);
  const int64_t blocks = (int64_t)B * nchunk * nkeyblk;
  MVK_REQUIRE(blocks < CSR_LIMIT, "%s: too many elements", what);
  hipLaunchKernelGGL((ordered_bwd_k<T, INTERP, CH>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, gc, gb,
                     w, row_start, entries, C, nv, hw, L, (int64_t)B * L, (int)nchunk, (int)nkeyblk, out, s);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

// feature_interpolate and group_points: grad_out (B, C, N2) or (B, C, N2*K), grad_in (B, C, N1)
template <typename T, bool INTERP>
int index_bwd_entry(const char* what, const T* g, const T* w, const int32_t* row_start, const int32_t* entries, int B,
                    int C, int64_t N1, int64_t N2, int K, T* gi, void* stream) {
  MVK_REQUIRE(B >= 0 && C >= 0 && N1 >= 0 && N2 >= 0 && K >= 0, "%s: bad sizes", what);
  const int64_t L = N2 * K, G = INTERP ? N2 : L;
  MVK_REQUIRE((int64_t)B * L < CSR_LIMIT && (int64_t)B * N1 < CSR_LIMIT, "%s: B*N2*K and B*N1 must be below 2^31", what);
  return ordered_bwd_entry<T, INTERP>(what, g, G, C * G, w, row_start, entries, B, C, 1, N1, L, gi,
                                      MapStrides{C * N1, N1, 1}, stream);
}

}  // namespace

extern "C" int64_t mvk_index_csr_workspace(int B, int64_t L, int64_t N1) {
  if (B < 0 || L < 0 || N1 < 0 || (int64_t)B * N1 >= CSR_LIMIT) return 0;
  const int64_t R = (int64_t)B * N1;
  return (R + csr_scan_blocks(R)) * (int64_t)sizeof(int32_t);
}

extern "C" int mvk_index_csr(const int64_t* index, int B, int64_t L, int64_t N1, int32_t* row_start, int32_t* entries,
                             int32_t* status, void* workspace, int64_t workspace_bytes, void* stream) {
  MVK_REQUIRE(B >= 0 && L >= 0 && N1 >= 0, "index_csr: bad sizes B=%d L=%lld N1=%lld", B, (long long)L, (long long)N1);
  const int64_t total = (int64_t)B * L, R = (int64_t)B * N1;
  MVK_REQUIRE(total < CSR_LIMIT && R < CSR_LIMIT, "index_csr: B*L = %lld and B*N1 = %lld must be below 2^31",
              (long long)total, (long long)R);
  MVK_REQUIRE(row_start && (total == 0 || (index && entries)), "index_csr: null operand");
  const int64_t need = mvk_index_csr_workspace(B, L, N1);
  MVK_REQUIRE(workspace && workspace_bytes >= need, "index_csr: the workspace needs %lld bytes (got %lld)",
              (long long)need, (long long)workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  int32_t* cursor = (int32_t*)workspace;
  int32_t* block_sums = cursor + R;
  const int64_t nblk = csr_scan_blocks(R);
  const int64_t zb = cdiv64(R + 1, CSR_T);
  hipLaunchKernelGGL(csr_zero_k, dim3((unsigned)(zb < 4096 ? zb : 4096)), dim3(CSR_T), 0, st, row_start, R + 1, cursor, R);
  const unsigned eb = (unsigned)cdiv64(total, CSR_T);
  if (total > 0)
    hipLaunchKernelGGL(csr_count_k, dim3(eb), dim3(CSR_T), 0, st, index, total, L, N1, row_start, status);
  hipLaunchKernelGGL(csr_block_sums_k, dim3((unsigned)nblk), dim3(TPB), 0, st, row_start, R + 1, block_sums);
  hipLaunchKernelGGL(csr_scan_sums_k, dim3(1), dim3(COMPACT_T), 0, st, block_sums, (int)nblk);
  hipLaunchKernelGGL(csr_scan_apply_k, dim3((unsigned)nblk), dim3(TPB), 0, st, row_start, R + 1, block_sums);
  if (total > 0 && R > 0) {
    hipLaunchKernelGGL(csr_fill_k, dim3(eb), dim3(CSR_T), 0, st, index, total, L, N1, row_start, cursor, entries);
    hipLaunchKernelGGL(csr_sort_k, dim3((unsigned)cdiv64(R, CSR_ROWS)), dim3(CSR_T), 0, st, index, R, L, N1, total,
                       row_start, entries);
  }
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_interpolate_bwd_csr(const float* grad_out, const float* weight, const int32_t* row_start,
                                       const int32_t* entries, int B, int C, int64_t N1, int64_t N2, float* grad_in,
                                       void* stream) {
  return index_bwd_entry<float, true>("interpolate_bwd_csr", grad_out, weight, row_start, entries, B, C, N1, N2, 3,
                                        grad_in, stream);
}
extern "C" int mvk_interpolate_bwd_csr_f64(const double* grad_out, const double* weight, const int32_t* row_start,
                                           const int32_t* entries, int B, int C, int64_t N1, int64_t N2, double* grad_in,
                                           void* stream) {
  return index_bwd_entry<double, true>("interpolate_bwd_csr", grad_out, weight, row_start, entries, B, C, N1, N2, 3,
                                         grad_in, stream);
}
extern "C" int mvk_group_points_bwd_csr(const float* grad_out, const int32_t* row_start, const int32_t* entries, int B,
                                        int C, int64_t N1, int64_t N2, int K, float* grad_in, void* stream) {
  return index_bwd_entry<float, false>("group_points_bwd_csr", grad_out, nullptr, row_start, entries, B, C, N1, N2, K,
                                         grad_in, stream);
}
extern "C" int mvk_group_points_bwd_csr_f64(const double* grad_out, const int32_t* row_start, const int32_t* entries, int B,
                                            int C, int64_t N1, int64_t N2, int K, double* grad_in, void* stream) {
  return index_bwd_entry<double, false>("group_points_bwd_csr", grad_out, nullptr, row_start, entries, B, C, N1, N2, K,
                                          grad_in, stream);
}

// The feature gradients of the training-mode row builders (pn2_rows.hip): dX is the channel-major operand [C.., B*L].
extern "C" int mvk_pn2_sa_rows_bwd_csr(const float* dX, const int32_t* row_start, const int32_t* entries, int B, int C,
                                       int64_t N, int64_t M, int K, float* dfeature, void* stream) {
  int64_t R;
  if (int rc = rows_sizes("pn2_sa_rows_bwd_csr", B, C, N, M, K, &R)) return rc;
  const int64_t L = M * (int64_t)K;
  return ordered_bwd_entry<float, false>("pn2_sa_rows_bwd_csr", dX, R, L, nullptr, row_start, entries, B, C, 1, N, L,
                                         dfeature, MapStrides{C * N, N, 1}, stream);
}
extern "C" int mvk_pn2_fa_rows_bwd_csr(const float* dX, const int32_t* row_start, const int32_t* entries, int B, int nv,
                                       int C, int64_t HW, int64_t N, int K, float* dfeature_2d, int64_t stride_image,
                                       int64_t stride_channel, int64_t stride_pixel, void* stream) {
  const MapStrides s{stride_image, stride_channel, stride_pixel};
  int64_t R, P;
  if (int rc = fa_sizes("pn2_fa_rows_bwd_csr", B, nv, C, HW, N, K, s, &R, &P)) return rc;
  const int64_t L = N * (int64_t)K;
  return ordered_bwd_entry<float, false>("pn2_fa_rows_bwd_csr", dX, R, L, nullptr, row_start, entries, B, C, nv, HW, L,
                                         dfeature_2d, s, stream);
}
