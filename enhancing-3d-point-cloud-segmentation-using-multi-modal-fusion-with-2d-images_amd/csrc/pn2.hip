// The point ops of the MVPNet baseline's PointNet++ (reference: mvpnet/ops/cuda/fps_kernel.cu:60-135,
// ball_query_kernel.cu:59-135, ball_query_distance_kernel.cu:59-137, knn_distance_kernel.cu:35-124,
// interpolate_kernel.cu:25-68 and :131-174), float32 and float64 like the reference's dispatch.
//
// Distances are formed in the input dtype as ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded: this file is
// compiled with -ffp-contract=off (no FMA), which is what the NumPy restatements in the reference's own tests compute.
//
//   fps_reg_k      farthest point sampling, one workgroup per cloud, up to 1024 lanes. Coordinates and running distances
//                  of a lane's points stay in registers for all rounds (PPL points per lane, lane t owns points
//                  t + i * blockDim): a round reads no global memory. The argmax is a lexicographic maximum over
//                  (distance, tie key): xor-shuffles within a wave, then one LDS slot per wave in a double-buffered
//                  table, one barrier per round; the winner's coordinates travel with its key through the slot.
//   fps_ws_k       the same rounds for clouds too large for registers: running distances in a caller-provided
//                  workspace, coordinates re-read (L2). Same picks.
//   Tie rule (what the reference's strided scan + LDS tree picks): with Bk the REFERENCE's block size
//                  (min(512, 2^floor(log2 N)), 16 below 16 points), among points of equal largest distance the one with
//                  the smallest bitreverse(j mod Bk, log2 Bk) wins, among those the smallest j. Here: tie key
//                  (bitreverse << 23) | j, smaller wins; blockDim is a power of two >= Bk, so all points of one lane
//                  share j mod Bk and the in-lane scan in ascending j with a strict > is the rule restricted to a lane.
//                  A point at distance 0 never wins; when no point has a positive distance the index is repeated.
//   Ragged form   (mvk_fps_ragged, mvk_pn2_ball_query_ragged): `lengths` [B] int64 or null. Cloud b is the rows [0, n_b)
//                  of its padded [N] block, n_b = clamp(lengths[b], 1, N): one load per workgroup (per wave in the ball
//                  query), uniform over the wave. Rows at or beyond n_b are never read. Thread count, points per lane,
//                  workspace and lb stay those of the padded N; the picks are still those of the n_b-point cloud alone:
//                  for j < n <= N the key built from Bk(N) orders points as the key from Bk(n) does. Bk(n) divides
//                  Bk(N), so bitreverse(j mod Bk(N)) has bitreverse(j mod Bk(n)) in its top bits, and what follows below
//                  them are the bits of j above log2 Bk(n), reversed. Below the cap of 512, n < 2 Bk(n): j < n has at most
//                  one such bit, and both keys compare it last (as that bit here, as part of j there). At the cap
//                  Bk(n) = Bk(N) = 512. Below 16 points Bk(n) = 16 > j, and the key from Bk(N) is bitreverse(j, 4)
//                  followed by zeros. (tests/test_pn2_ragged_cpu.py checks this on lattice clouds.)
//   ball_query_k   one wave per query, 64 consecutive keys per round: ballot, prefix popcount, ordered write; stops once
//                  K hits are found. No barrier (a wave leaves early on its own).
//   knn3_k         one lane per query, key tiles staged in LDS, three sorted slots updated by strict-< insertion.
//   interp_*_k     one lane per (b, c, n); the backward is a scatter-add with float atomics (not deterministic in order;
//                  its fixed-order form is mvk_interpolate_bwd_csr in pn2_ordered.hip).
#include <limits>

#include "common.h"

namespace {

constexpr int FPS_MAX_T = 1024;
constexpr int FPS_MAX_WAVES = FPS_MAX_T / 64;
constexpr int FPS_J_BITS = 23;                      // tie key = (bitreverse << 23) | j
constexpr uint32_t FPS_NO_KEY = 0xFFFFFFFFu;

template <typename T>
__device__ __forceinline__ bool cand_better(T da, uint32_t ka, T db, uint32_t kb) {
  return da > db || (da == db && ka < kb);
}

template <typename T, int D>
__device__ __forceinline__ T dist2(T ax, T ay, T az, T bx, T by, T bz) {
  const T dx = ax - bx, dy = ay - by;
  T d = (dx * dx) + (dy * dy);
  if (D == 3) {
    const T dz = az - bz;
    d = d + (dz * dz);
  }
  return d;
}

template <typename T>
struct FpsShared {
  T d[2][FPS_MAX_WAVES];
  uint32_t k[2][FPS_MAX_WAVES];
  T c[2][FPS_MAX_WAVES][3];
};

// A lane's candidate (bd > 0 with key bk and coordinates bx.., or bd == 0: none) -> the workgroup's winner. Returns true
// and sets cur / c* when some point has a positive distance. One barrier; `buf` alternates between rounds.
template <typename T>
__device__ __forceinline__ bool fps_pick(FpsShared<T>& sh, int buf, T bd, uint32_t bk, T bx, T by, T bz, int64_t& cur,
                                         T& cx, T& cy, T& cz) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  T wd = bd;
  uint32_t wk = bk;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T od = __shfl_xor(wd, off, 64);
    const uint32_t ok = (uint32_t)__shfl_xor((int)wk, off, 64);
    if (cand_better(od, ok, wd, wk)) {
      wd = od;
      wk = ok;
    }
  }
  if (wd > (T)0) {
    if (bd > (T)0 && bk == wk) {                    // keys are unique per point: exactly one lane
      sh.d[buf][wave] = bd;
      sh.k[buf][wave] = bk;
      sh.c[buf][wave][0] = bx;
      sh.c[buf][wave][1] = by;
      sh.c[buf][wave][2] = bz;
    }
  } else if (lane == 0) {
    sh.d[buf][wave] = (T)0;
    sh.k[buf][wave] = FPS_NO_KEY;
  }
  __syncthreads();
  T gd = sh.d[buf][0];
  uint32_t gk = sh.k[buf][0];
  int gw = 0;
  for (int w = 1; w < nw; ++w) {
    const T od = sh.d[buf][w];
    const uint32_t ok = sh.k[buf][w];
    if (cand_better(od, ok, gd, gk)) {
      gd = od;
      gk = ok;
      gw = w;
    }
  }
  if (!(gd > (T)0)) return false;
  cur = (int64_t)(gk & ((1u << FPS_J_BITS) - 1));
  cx = sh.c[buf][gw][0];
  cy = sh.c[buf][gw][1];
  cz = sh.c[buf][gw][2];
  return true;
}

// The point count of cloud b: N without `lengths`, else lengths[b] clamped to [1, N] (see "Ragged form" above).
__device__ __forceinline__ int64_t ragged_len(const int64_t* __restrict__ lengths, int64_t b, int64_t N) {
  if (!lengths) return N;
  const int64_t n = lengths[b];
  return n < 1 ? 1 : (n > N ? N : n);
}

__device__ __forceinline__ uint32_t fps_rev(int64_t j, int lb) {
  return __brev((uint32_t)j & ((1u << lb) - 1)) >> (32 - lb);
}

template <typename T, int D, int PPL>
__global__ __launch_bounds__(FPS_MAX_T) void fps_reg_k(const T* __restrict__ points, const int64_t* __restrict__ lengths,
                                                       int64_t N, int64_t M, int lb, int64_t* __restrict__ index) {
  __shared__ FpsShared<T> sh;
  const int t = threadIdx.x, nt = blockDim.x;
  const T* P = points + (int64_t)blockIdx.x * N * D;
  int64_t* out = index + (int64_t)blockIdx.x * M;
  const int64_t nb = ragged_len(lengths, blockIdx.x, N);
  T px[PPL], py[PPL], pz[PPL], run[PPL];
#pragma unroll
  for (int i = 0; i < PPL; ++i) {
    const int64_t j = t + (int64_t)i * nt;
    const bool valid = j < nb;
    px[i] = valid ? P[j * D] : (T)0;
    py[i] = valid ? P[j * D + 1] : (T)0;
    pz[i] = (valid && D == 3) ? P[j * D + 2] : (T)0;
    run[i] = valid ? std::numeric_limits<T>::infinity() : (T)0;      // a lane's padding has distance 0: never wins
  }
  const uint32_t rev = fps_rev(t, lb) << FPS_J_BITS;                 // blockDim is a multiple of 2^lb
  int64_t cur = 0;
  T cx = P[0], cy = P[1], cz = D == 3 ? P[2] : (T)0;
  if (t == 0) out[0] = 0;
  for (int64_t r = 1; r < M; ++r) {
    T bd = (T)0, bx = (T)0, by = (T)0, bz = (T)0;
    int bi = 0;
#pragma unroll
    for (int i = 0; i < PPL; ++i) {
      T d = dist2<T, D>(px[i], py[i], pz[i], cx, cy, cz);
      d = run[i] > d ? d : run[i];
      run[i] = d;
      if (d > bd) {
        bd = d;
        bi = i;
        bx = px[i];
        by = py[i];
        bz = pz[i];
      }
    }
    const uint32_t bk = bd > (T)0 ? (rev | (uint32_t)(t + bi * nt)) : FPS_NO_KEY;
    fps_pick<T>(sh, (int)(r & 1), bd, bk, bx, by, bz, cur, cx, cy, cz);
    if (t == 0) out[r] = cur;
  }
}

template <typename T, int D>
__global__ __launch_bounds__(FPS_MAX_T) void fps_ws_k(const T* __restrict__ points, const int64_t* __restrict__ lengths,
                                                      int64_t N, int64_t M, int lb, T* __restrict__ ws,
                                                      int64_t* __restrict__ index) {
  __shared__ FpsShared<T> sh;
  const int t = threadIdx.x, nt = blockDim.x;
  const T* P = points + (int64_t)blockIdx.x * N * D;
  T* run = ws + (int64_t)blockIdx.x * N;
  int64_t* out = index + (int64_t)blockIdx.x * M;
  const int64_t nb = ragged_len(lengths, blockIdx.x, N);
  const uint32_t rev = fps_rev(t, lb) << FPS_J_BITS;
  int64_t cur = 0;
  T cx = P[0], cy = P[1], cz = D == 3 ? P[2] : (T)0;
  if (t == 0) out[0] = 0;
  for (int64_t r = 1; r < M; ++r) {
    T bd = (T)0, bx = (T)0, by = (T)0, bz = (T)0;
    int64_t bj = 0;
    for (int64_t j = t; j < nb; j += nt) {                           // a slot of `run` is only ever touched by its lane
      const T x = P[j * D], y = P[j * D + 1], z = D == 3 ? P[j * D + 2] : (T)0;
      T d = dist2<T, D>(x, y, z, cx, cy, cz);
      if (r > 1) {
        const T last = run[j];
        d = last > d ? d : last;
      }
      run[j] = d;
      if (d > bd) {
        bd = d;
        bj = j;
        bx = x;
        by = y;
        bz = z;
      }
    }
    const uint32_t bk = bd > (T)0 ? (rev | (uint32_t)bj) : FPS_NO_KEY;
    fps_pick<T>(sh, (int)(r & 1), bd, bk, bx, by, bz, cur, cx, cy, cz);
    if (t == 0) out[r] = cur;
  }
}

// ------------------------------------------------------------------------------------------------------------------

constexpr int BQ_T = 256;                            // 4 waves = 4 queries per workgroup

template <typename T>
__global__ __launch_bounds__(BQ_T) void ball_query_k(const T* __restrict__ query, const T* __restrict__ key,
                                                     const int64_t* __restrict__ lengths, int64_t total, int64_t N1,
                                                     int64_t N2, T r2, int K, int64_t* __restrict__ index,
                                                     T* __restrict__ distance) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * (BQ_T / 64) + (threadIdx.x >> 6);
  if (q >= total) return;                            // whole waves leave; the kernel has no barrier
  const int64_t b = q / N1;
  const T qx = query[q * 3], qy = query[q * 3 + 1], qz = query[q * 3 + 2];
  const T* Kp = key + b * N2 * 3;
  const int64_t nb = ragged_len(lengths, b, N2);       // the keys of batch element b: rows [0, nb)
  int64_t* out = index + q * K;
  T* dout = distance ? distance + q * K : nullptr;
  int cnt = 0;
  int64_t first = -1;
  for (int64_t base = 0; base < nb && cnt < K; base += 64) {
    const int64_t j = base + lane;
    bool hit = false;
    T d = (T)0;
    if (j < nb) {
      d = dist2<T, 3>(Kp[j * 3], Kp[j * 3 + 1], Kp[j * 3 + 2], qx, qy, qz);
      hit = d < r2;
    }
    const unsigned long long mask = __ballot(hit);
    if (mask == 0) continue;
    if (first < 0) first = base + (__ffsll((long long)mask) - 1);
    const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
    if (hit && pos < K) {
      out[pos] = j;
      if (dout) dout[pos] = d;
    }
    cnt += __popcll(mask);
  }
  if (cnt > K) cnt = K;
  for (int s = cnt + lane; s < K; s += 64) {         // ball_query_kernel.cu:128-133; no hit: the -1 of at::full
    out[s] = first;
    if (dout) dout[s] = (T)-1;
  }
}

constexpr int KNN_T = 256;

template <typename T>
__global__ __launch_bounds__(KNN_T) void knn3_k(const T* __restrict__ query, const T* __restrict__ key, int64_t N1,
                                                int64_t N2, int64_t* __restrict__ index, T* __restrict__ distance) {
  __shared__ T s_key[KNN_T * 3];
  const int64_t b = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * KNN_T + threadIdx.x;
  const bool active = n < N1;
  const T* Kp = key + b * N2 * 3;
  T qx = (T)0, qy = (T)0, qz = (T)0;
  if (active) {
    const T* Q = query + (b * N1 + n) * 3;
    qx = Q[0];
    qy = Q[1];
    qz = Q[2];
  }
  const T inf = std::numeric_limits<T>::infinity();
  T d0 = inf, d1 = inf, d2 = inf;
  int64_t i0 = -1, i1 = -1, i2 = -1;
  for (int64_t base = 0; base < N2; base += KNN_T) {
    const int tile = (int)((N2 - base) < KNN_T ? (N2 - base) : KNN_T);
    for (int e = threadIdx.x; e < tile * 3; e += KNN_T) s_key[e] = Kp[base * 3 + e];
    __syncthreads();
    if (active) {
      for (int jj = 0; jj < tile; ++jj) {
        const T d = dist2<T, 3>(s_key[jj * 3], s_key[jj * 3 + 1], s_key[jj * 3 + 2], qx, qy, qz);
        const int64_t j = base + jj;
        if (d < d0) {                                // knn_distance_kernel.cu:97-106: strict <, the earlier key keeps a tie
          d2 = d1; i2 = i1;
          d1 = d0; i1 = i0;
          d0 = d;  i0 = j;
        } else if (d < d1) {
          d2 = d1; i2 = i1;
          d1 = d;  i1 = j;
        } else if (d < d2) {
          d2 = d;  i2 = j;
        }
      }
    }
    __syncthreads();
  }
  if (active) {
    int64_t* io = index + (b * N1 + n) * 3;
    T* dd = distance + (b * N1 + n) * 3;
    io[0] = i0; io[1] = i1; io[2] = i2;
    dd[0] = d0; dd[1] = d1; dd[2] = d2;
  }
}

constexpr int IT = 256;

template <typename T>
__global__ __launch_bounds__(IT) void interp_fwd_k(const T* __restrict__ feature, const int64_t* __restrict__ index,
                                                   const T* __restrict__ weight, int64_t total, int C, int64_t N1,
                                                   int64_t N2, T* __restrict__ out, int32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * IT + threadIdx.x;
  if (e >= total) return;
  const int64_t n = e % N2, bc = e / N2, b = bc / C;
  const int64_t* ix = index + (b * N2 + n) * 3;
  const T* w = weight + (b * N2 + n) * 3;
  const T* f = feature + bc * N1;
  T acc = (T)0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t j = ix[k];
    if (j >= 0 && j < N1)
      acc = acc + f[j] * w[k];
    else
      bad = true;
  }
  out[e] = acc;
  if (bad && status) *status = 1;
}

template <typename T>
__global__ __launch_bounds__(IT) void interp_bwd_k(const T* __restrict__ grad_out, const int64_t* __restrict__ index,
                                                   const T* __restrict__ weight, int64_t total, int C, int64_t N1,
                                                   int64_t N2, T* __restrict__ grad_in, int32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * IT + threadIdx.x;
  if (e >= total) return;
  const int64_t n = e % N2, bc = e / N2, b = bc / C;
  const int64_t* ix = index + (b * N2 + n) * 3;
  const T* w = weight + (b * N2 + n) * 3;
  const T g = grad_out[e];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t j = ix[k];
    if (j >= 0 && j < N1)
      atomicAdd(grad_in + bc * N1 + j, g * w[k]);    // interpolate_kernel.cu:171
    else
      bad = true;
  }
  if (bad && status) *status = 1;
}

// ------------------------------------------------------------------------------------------------------------------

inline int fps_ref_log2_block(int64_t N) {           // log2 of the reference's block size (fps_kernel.cu:21-24, :166-175)
  int lb = 0;
  while (lb < 9 && ((int64_t)2 << lb) <= N) ++lb;
  return lb < 4 ? 4 : lb;
}

inline int fps_threads(int64_t N) {                  // power of two in [64, 1024]: a multiple of the reference's block size
  int t = 64;
  while (t < FPS_MAX_T && t < N) t <<= 1;
  return t;
}

template <typename T>
constexpr int fps_max_ppl() { return sizeof(T) == 8 ? 8 : 16; }   // registers: 4 values per point, 128 VGPRs at 1024 lanes

template <typename T>
inline int64_t fps_workspace_bytes(int64_t B, int64_t N) {
  return N <= (int64_t)FPS_MAX_T * fps_max_ppl<T>() ? 0 : B * N * (int64_t)sizeof(T);
}

template <typename T, int D>
int fps_launch(const T* points, const int64_t* lengths, int B, int64_t N, int64_t M, int64_t* index, void* ws,
               int64_t ws_bytes, hipStream_t st) {
  const int lb = fps_ref_log2_block(N), nt = fps_threads(N);
  const int64_t ppl = cdiv64(N, nt);
#define MVK_FPS_REG(P)                                                                                            \
  if (ppl <= P) {                                                                                                 \
    hipLaunchKernelGGL((fps_reg_k<T, D, P>), dim3((unsigned)B), dim3(nt), 0, st, points, lengths, N, M, lb, index); \
    MVK_CHECK_HIP(hipGetLastError());                                                                             \
    return 0;                                                                                                     \
  }
  MVK_FPS_REG(1)
  MVK_FPS_REG(2)
  MVK_FPS_REG(4)
  MVK_FPS_REG(8)
  if constexpr (fps_max_ppl<T>() >= 16) {
    MVK_FPS_REG(16)
  }
#undef MVK_FPS_REG
  const int64_t need = fps_workspace_bytes<T>(B, N);
  MVK_REQUIRE(ws && ws_bytes >= need, "fps: %lld points per cloud need a workspace of %lld bytes (got %lld)",
              (long long)N, (long long)need, (long long)ws_bytes);
  hipLaunchKernelGGL((fps_ws_k<T, D>), dim3((unsigned)B), dim3(FPS_MAX_T), 0, st, points, lengths, N, M, lb, (T*)ws,
                     index);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int fps_entry(const T* points, const int64_t* lengths, int B, int64_t N, int D, int64_t M, int64_t* index, void* ws,
              int64_t ws_bytes, void* stream) {
  MVK_REQUIRE(B >= 0 && N >= 1 && N < ((int64_t)1 << FPS_J_BITS), "fps: bad sizes B=%d N=%lld (1 <= N < 2^%d)", B,
              (long long)N, FPS_J_BITS);
  MVK_REQUIRE(D == 2 || D == 3, "fps: only 2-D and 3-D points (got D=%d)", D);
  MVK_REQUIRE(M >= 1 && M <= N, "fps: %lld centroids of %lld points (need 1 <= M <= N)", (long long)M, (long long)N);
  if (B == 0) return 0;
  MVK_REQUIRE(points && index, "fps: null operand");
  hipStream_t st = (hipStream_t)stream;
  return D == 3 ? fps_launch<T, 3>(points, lengths, B, N, M, index, ws, ws_bytes, st)
                : fps_launch<T, 2>(points, lengths, B, N, M, index, ws, ws_bytes, st);
}

template <typename T>
int ball_query_entry(const T* query, const T* key, const int64_t* lengths, int B, int64_t N1, int64_t N2, float radius,
                     int K, int64_t* index, T* distance, void* stream) {
  MVK_REQUIRE(B >= 0 && N1 >= 0 && N2 >= 1 && K >= 1, "pn2_ball_query: bad sizes B=%d N1=%lld N2=%lld K=%d", B,
              (long long)N1, (long long)N2, K);
  const int64_t total = (int64_t)B * N1;
  if (total == 0) return 0;
  MVK_REQUIRE(query && key && index, "pn2_ball_query: null operand");
  MVK_REQUIRE(total < ((int64_t)1 << 31), "pn2_ball_query: too many queries");
  const T r = (T)radius;                              // ball_query_kernel.cu:45,73
  const T r2 = r * r;
  hipLaunchKernelGGL(ball_query_k<T>, dim3((unsigned)cdiv64(total, BQ_T / 64)), dim3(BQ_T), 0, (hipStream_t)stream, query,
                     key, lengths, total, N1, N2, r2, K, index, distance);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int knn_entry(const T* query, const T* key, int B, int64_t N1, int64_t N2, int k, int64_t* index, T* distance,
              void* stream) {
  MVK_REQUIRE(k == 3, "knn_distance: only 3-NN is supported (got k=%d)", k);
  MVK_REQUIRE(B >= 0 && B < 65536 && N1 >= 0, "knn_distance: bad sizes B=%d N1=%lld", B, (long long)N1);
  MVK_REQUIRE(N2 >= k, "knn_distance: %lld keys for k=%d", (long long)N2, k);
  if (B == 0 || N1 == 0) return 0;
  MVK_REQUIRE(query && key && index && distance, "knn_distance: null operand");
  hipLaunchKernelGGL(knn3_k<T>, dim3((unsigned)cdiv64(N1, KNN_T), (unsigned)B), dim3(KNN_T), 0, (hipStream_t)stream, query,
                     key, N1, N2, index, distance);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

template <typename T, bool BWD>
int interp_entry(const T* src, const int64_t* index, const T* weight, int B, int C, int64_t N1, int64_t N2, T* dst,
                 int32_t* status, void* stream) {
  MVK_REQUIRE(B >= 0 && C >= 0 && N1 >= 0 && N2 >= 0, "interpolate: bad sizes");
  const int64_t total = (int64_t)B * C * N2;
  if (total == 0) return 0;
  MVK_REQUIRE(src && index && weight && dst, "interpolate: null operand");
  MVK_REQUIRE(total < ((int64_t)1 << 31) * IT, "interpolate: too many elements");
  const unsigned gx = (unsigned)cdiv64(total, IT);
  if (BWD)
    hipLaunchKernelGGL(interp_bwd_k<T>, dim3(gx), dim3(IT), 0, (hipStream_t)stream, src, index, weight, total, C, N1, N2,
                       dst, status);
  else
    hipLaunchKernelGGL(interp_fwd_k<T>, dim3(gx), dim3(IT), 0, (hipStream_t)stream, src, index, weight, total, C, N1, N2,
                       dst, status);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int64_t mvk_fps_workspace(int64_t B, int64_t N, int f64) {
  if (B < 0 || N < 0) return 0;
  return f64 ? fps_workspace_bytes<double>(B, N) : fps_workspace_bytes<float>(B, N);
}

extern "C" int mvk_fps(const float* points, int B, int64_t N, int D, int64_t M, int64_t* index, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  return fps_entry<float>(points, nullptr, B, N, D, M, index, workspace, workspace_bytes, stream);
}
extern "C" int mvk_fps_f64(const double* points, int B, int64_t N, int D, int64_t M, int64_t* index, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  return fps_entry<double>(points, nullptr, B, N, D, M, index, workspace, workspace_bytes, stream);
}

extern "C" int mvk_fps_ragged(const float* points, const int64_t* lengths, int B, int64_t N, int D, int64_t M,
                              int64_t* index, void* workspace, int64_t workspace_bytes, void* stream) {
  MVK_REQUIRE(lengths || B <= 0, "fps_ragged: null lengths");
  return fps_entry<float>(points, lengths, B, N, D, M, index, workspace, workspace_bytes, stream);
}
extern "C" int mvk_fps_ragged_f64(const double* points, const int64_t* lengths, int B, int64_t N, int D, int64_t M,
                                  int64_t* index, void* workspace, int64_t workspace_bytes, void* stream) {
  MVK_REQUIRE(lengths || B <= 0, "fps_ragged: null lengths");
  return fps_entry<double>(points, lengths, B, N, D, M, index, workspace, workspace_bytes, stream);
}

extern "C" int mvk_pn2_ball_query(const float* query, const float* key, int B, int64_t N1, int64_t N2, float radius, int K,
                                  int64_t* index, float* distance, void* stream) {
  return ball_query_entry<float>(query, key, nullptr, B, N1, N2, radius, K, index, distance, stream);
}
extern "C" int mvk_pn2_ball_query_f64(const double* query, const double* key, int B, int64_t N1, int64_t N2, float radius,
                                      int K, int64_t* index, double* distance, void* stream) {
  return ball_query_entry<double>(query, key, nullptr, B, N1, N2, radius, K, index, distance, stream);
}

extern "C" int mvk_pn2_ball_query_ragged(const float* query, const float* key, const int64_t* key_lengths, int B,
                                         int64_t N1, int64_t N2, float radius, int K, int64_t* index, float* distance,
                                         void* stream) {
  MVK_REQUIRE(key_lengths || B <= 0 || N1 <= 0, "pn2_ball_query_ragged: null key_lengths");
  return ball_query_entry<float>(query, key, key_lengths, B, N1, N2, radius, K, index, distance, stream);
}
extern "C" int mvk_pn2_ball_query_ragged_f64(const double* query, const double* key, const int64_t* key_lengths, int B,
                                             int64_t N1, int64_t N2, float radius, int K, int64_t* index,
                                             double* distance, void* stream) {
  MVK_REQUIRE(key_lengths || B <= 0 || N1 <= 0, "pn2_ball_query_ragged: null key_lengths");
  return ball_query_entry<double>(query, key, key_lengths, B, N1, N2, radius, K, index, distance, stream);
}

extern "C" int mvk_knn_distance(const float* query, const float* key, int B, int64_t N1, int64_t N2, int k, int64_t* index,
                                float* distance, void* stream) {
  return knn_entry<float>(query, key, B, N1, N2, k, index, distance, stream);
}
extern "C" int mvk_knn_distance_f64(const double* query, const double* key, int B, int64_t N1, int64_t N2, int k,
                                    int64_t* index, double* distance, void* stream) {
  return knn_entry<double>(query, key, B, N1, N2, k, index, distance, stream);
}

extern "C" int mvk_interpolate_fwd(const float* feature, const int64_t* index, const float* weight, int B, int C,
                                   int64_t N1, int64_t N2, float* out, int32_t* status, void* stream) {
  return interp_entry<float, false>(feature, index, weight, B, C, N1, N2, out, status, stream);
}
extern "C" int mvk_interpolate_fwd_f64(const double* feature, const int64_t* index, const double* weight, int B, int C,
                                       int64_t N1, int64_t N2, double* out, int32_t* status, void* stream) {
  return interp_entry<double, false>(feature, index, weight, B, C, N1, N2, out, status, stream);
}
extern "C" int mvk_interpolate_bwd(const float* grad_out, const int64_t* index, const float* weight, int B, int C,
                                   int64_t N1, int64_t N2, float* grad_in, int32_t* status, void* stream) {
  return interp_entry<float, true>(grad_out, index, weight, B, C, N1, N2, grad_in, status, stream);
}
extern "C" int mvk_interpolate_bwd_f64(const double* grad_out, const int64_t* index, const double* weight, int B, int C,
                                       int64_t N1, int64_t N2, double* grad_in, int32_t* status, void* stream) {
  return interp_entry<double, true>(grad_out, index, weight, B, C, N1, N2, grad_in, status, stream);
}
