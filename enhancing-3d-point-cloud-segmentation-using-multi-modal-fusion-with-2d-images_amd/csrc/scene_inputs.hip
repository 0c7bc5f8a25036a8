// The inputs of the MVPNet whole-scene test for G chunks at a time (include/mvkpconv_scene.h; reference:
// mvpnet/data/scannet_2d3d.py:199-321, mvpnet/test_mvpnet_3d.py:153-158). One chunk at a time this is
// mvpnet/test_mvpnet_3d.py:chunk_rgbd_inputs: about fifteen tensor operations, seven k-NN launches and num_rgbd_frames + 1
// reads back per chunk. Here a group goes from "scene, frames and chunk CSR in HBM" to the padded batch without a read:
//   overlap_pack_k      the (nb, nf) overlap table as frame-major bit rows, once per scene
//   select_frames_k     greedy maximum coverage, one workgroup per chunk: the chunk's base points as a bit mask in LDS
//                       (a binary search of base_point_ind[b] in the chunk's ascending CSR row, 64 base points per ballot),
//                       then nv rounds of popcount(row_f & alive) summed per wave, first maximum, alive &= ~row_pick
//   chunk_unproject_k   unprojection of the chosen frames (csrc/unproject.h: fusion.hip's expression), the strict float64
//                       box mask, the float32 copy, the image planes and the count of valid pixels
//   chunk_queries_k     the chunks' own points, gathered once: the k-NN queries and the source of the batch's points
//   chunk_batch_rows_k  points [G,3,n_max] and knn_indices [G,n_max,k] with a sparse chunk's pad rows and zero padding
// The k-NN itself is mvk_knn_f64 (csrc/fusion.hip), once per chunk on the same stream with one workspace.
// Integer arithmetic, or float64 in the written order (-ffp-contract=off). The only atomics are integer counters summed
// in LDS first. A workgroup never straddles two chunks, so per-chunk values are read at wave-uniform addresses.
#include "common.h"
#include "select_frames.h"
#include "unproject.h"
#include "../../include/mvkpconv_scene.h"

namespace {

constexpr int OP_T = 256;        // threads of the pack kernel
constexpr int UP_T = 256;        // threads of the unprojection kernel
constexpr int BR_T = 256;        // threads of the gather kernels
constexpr int64_t MAX_GRID = ((int64_t)1 << 31) - 1;
constexpr int64_t MAX_SIZE = (int64_t)1 << 31;

// thread t -> (word w, frame f) with f fastest: neighbouring lanes read neighbouring bytes of one table row
__global__ __launch_bounds__(OP_T) void overlap_pack_k(const uint8_t* __restrict__ overlap, int64_t nb, int64_t nf,
                                                       int64_t W, uint32_t* __restrict__ packed) {
  const int64_t t = (int64_t)blockIdx.x * OP_T + threadIdx.x;
  if (t >= W * nf) return;
  const int64_t w = t / nf, f = t - w * nf;
  const int64_t b0 = w * 32;
  uint32_t bits = 0;
  for (int i = 0; i < 32; ++i)
    if (b0 + i < nb && overlap[(b0 + i) * nf + f] != 0) bits |= 1u << i;
  packed[f * W + w] = bits;
}

// LDS: alive [W] words | count [nf] int32 (dynamic), the pick (static). The choice itself is select_frames.h's.
__global__ __launch_bounds__(SF_T) void select_frames_k(const uint32_t* __restrict__ packed, int nb, int nf, int W,
                                                        const int64_t* __restrict__ base_point_ind,
                                                        const int64_t* __restrict__ rows, int64_t total,
                                                        const int64_t* __restrict__ row_off,
                                                        const int64_t* __restrict__ row_len, int nv,
                                                        int32_t* __restrict__ sel) {
  extern __shared__ uint32_t s_mem[];
  __shared__ int s_pick;
  const int g = blockIdx.x;
  int64_t j0 = row_off[g], n = row_len[g];
  if (j0 < 0 || j0 > total || n < 0) n = 0;               // a row that leaves the CSR is cut to it
  else if (n > total - j0) n = total - j0;
  select_frames_wg(packed, nb, nf, W, base_point_ind, 0, rows + (n > 0 ? j0 : 0), n, nv, sel + (int64_t)g * nv, s_mem,
                   (int*)(s_mem + W), &s_pick);
}

__global__ __launch_bounds__(UP_T) void chunk_unproject_k(const int32_t* __restrict__ sel, int nv,
                                                          const uint16_t* __restrict__ depth,
                                                          const float* __restrict__ images_in,
                                                          const float* __restrict__ poses, int nf, int h, int w,
                                                          int blocks_per_chunk, Cam cam,
                                                          const double* __restrict__ bounds, double* __restrict__ keys,
                                                          float* __restrict__ image_xyz, uint8_t* __restrict__ image_mask,
                                                          float* __restrict__ images_out, int32_t* __restrict__ num_valid) {
  __shared__ int s_n;
  const int g = blockIdx.x / blocks_per_chunk;                         // one chunk per workgroup
  const int64_t hw = (int64_t)h * w, P = (int64_t)nv * hw;
  const int64_t p = (int64_t)(blockIdx.x - g * blocks_per_chunk) * UP_T + threadIdx.x;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  bool valid = false;
  if (p < P) {
    const int view = (int)(p / hw);
    const int64_t pix = p - view * hw;
    const int f = sel[(int64_t)g * nv + view];
    const int64_t out = (int64_t)g * P + p;
    float rgb[3] = {0.f, 0.f, 0.f};
    double c[3] = {0.0, 0.0, 0.0}, x[3] = {0.0, 0.0, 0.0};
    if (f >= 0 && f < nf) {
      const int64_t src = (int64_t)f * hw + pix;
      unproject_pixel(cam, poses + (int64_t)f * 16, (double)(pix % w), (double)(pix / w), depth[src], c, x);
      const double* __restrict__ b = bounds + (int64_t)g * 4;          // wave-uniform
      valid = c[2] > 0.0 && x[0] > b[0] && x[0] < b[1] && x[1] > b[2] && x[1] < b[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) rgb[ch] = images_in[src * 3 + ch];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      keys[out * 3 + r] = x[r];
      image_xyz[out * 3 + r] = (float)x[r];
      images_out[(((int64_t)g * nv + view) * 3 + r) * hw + pix] = rgb[r];
    }
    image_mask[out] = valid ? 1 : 0;
  }
  const unsigned long long m = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_n, __popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(&num_valid[g], s_n);
}

// queries[q_off[g] + j] = points[rows[row_off[g] + j]]: thread t finds its chunk in the running sum
__global__ __launch_bounds__(BR_T) void chunk_queries_k(const float* __restrict__ points, int64_t N,
                                                        const int64_t* __restrict__ rows, int64_t total,
                                                        const int64_t* __restrict__ row_off,
                                                        const int64_t* __restrict__ q_off, int G, int64_t sum,
                                                        float* __restrict__ queries) {
  const int64_t t = (int64_t)blockIdx.x * BR_T + threadIdx.x;
  if (t >= sum) return;
  int lo = 0, hi = G;                                                  // the last g with q_off[g] <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (q_off[mid] <= t) lo = mid; else hi = mid;
  }
  const int64_t at = row_off[lo] + (t - q_off[lo]);
  int64_t i = at >= 0 && at < total ? rows[at] : -1;
  if (i < 0 || i >= N) i = -1;
#pragma unroll
  for (int c = 0; c < 3; ++c) queries[t * 3 + c] = i >= 0 ? points[i * 3 + c] : 0.f;
}

__global__ __launch_bounds__(BR_T) void chunk_batch_rows_k(const float* __restrict__ queries,
                                                           const int64_t* __restrict__ knn,
                                                           const int64_t* __restrict__ q_off,
                                                           const int64_t* __restrict__ row_len,
                                                           const int64_t* __restrict__ lengths,
                                                           const int32_t* __restrict__ extras,
                                                           const int64_t* __restrict__ extra_off, int blocks_per_chunk,
                                                           int64_t n_max, int k, float* __restrict__ points_out,
                                                           int64_t* __restrict__ knn_out) {
  const int g = blockIdx.x / blocks_per_chunk;                         // one chunk per workgroup
  const int64_t j = (int64_t)(blockIdx.x - g * blocks_per_chunk) * BR_T + threadIdx.x;
  if (j >= n_max) return;
  const int64_t nc = row_len[g], len = lengths[g];                     // wave-uniform
  int64_t r = -1;
  if (j < nc) r = j;
  else if (j < len) {
    const int64_t e = extra_off[g] + (j - nc);
    if (e < extra_off[g + 1]) r = extras[e];
  }
  if (r >= nc) r = -1;
  const int64_t q = r >= 0 ? q_off[g] + r : -1;
#pragma unroll
  for (int c = 0; c < 3; ++c) points_out[((int64_t)g * 3 + c) * n_max + j] = q >= 0 ? queries[q * 3 + c] : 0.f;
  for (int c = 0; c < k; ++c) knn_out[((int64_t)g * n_max + j) * k + c] = q >= 0 ? knn[q * k + c] : 0;
}

template <typename Kern>
int allow_lds(Kern kern, int64_t lds) {
  if (lds > 64 * 1024)
    MVK_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}

}  // namespace

extern "C" int mvk_overlap_pack(const uint8_t* overlap, int64_t nb, int64_t nf, int32_t* packed, void* stream) {
  MVK_REQUIRE(nb >= 0 && nf >= 0 && nb < MAX_SIZE && nf < MAX_SIZE && (nb == 0 || nf < MAX_SIZE / nb),
              "overlap_pack: bad sizes nb=%lld nf=%lld (nb * nf < 2^31)", (long long)nb, (long long)nf);
  if (nb == 0 || nf == 0) return 0;
  MVK_REQUIRE(overlap && packed, "overlap_pack: null operand");
  const int64_t W = cdiv64(nb, 32);
  hipLaunchKernelGGL(overlap_pack_k, dim3((unsigned)cdiv64(W * nf, OP_T)), dim3(OP_T), 0, (hipStream_t)stream, overlap, nb,
                     nf, W, (uint32_t*)packed);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_chunk_select_frames(const int32_t* packed, int64_t nb, int64_t nf, const int64_t* base_point_ind,
                                       const int64_t* rows, int64_t total, const int64_t* row_off, const int64_t* row_len,
                                       int G, int nv, int32_t* sel, void* stream) {
  MVK_REQUIRE(nb >= 0 && nf >= 0 && total >= 0 && G >= 0 && nv >= 0 && total < MAX_SIZE && (int64_t)G * nv < MAX_SIZE,
              "chunk_select_frames: bad sizes nb=%lld nf=%lld total=%lld G=%d nv=%d", (long long)nb, (long long)nf,
              (long long)total, G, nv);
  MVK_REQUIRE(nb <= MVK_SCENE_MAX_BASE && nf <= MVK_SCENE_MAX_FRAMES,
              "chunk_select_frames: nb=%lld base points (<= %d: the mask of a chunk's base points is 64 KiB of LDS) or nf=%lld "
              "frames (<= %d: their counts live in LDS) exceed the kernel's capacity; there is no fallback",
              (long long)nb, MVK_SCENE_MAX_BASE, (long long)nf, MVK_SCENE_MAX_FRAMES);
  if (G == 0 || nv == 0) return 0;
  MVK_REQUIRE(nf >= 1, "chunk_select_frames: no frame to choose from");
  MVK_REQUIRE(sel && row_off && row_len && (packed || nb == 0) && (base_point_ind || nb == 0) && (rows || total == 0),
              "chunk_select_frames: null operand");
  const int W = (int)cdiv64(nb, 32);
  const int64_t lds = ((int64_t)W + nf) * 4;
  if (allow_lds(select_frames_k, lds)) return -2;
  hipLaunchKernelGGL(select_frames_k, dim3(G), dim3(SF_T), (size_t)lds, (hipStream_t)stream, (const uint32_t*)packed, (int)nb,
                     (int)nf, W, base_point_ind, rows, total, row_off, row_len, nv, sel);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_chunk_unproject(const int32_t* sel, int G, int nv, const uint16_t* depth, const float* images_in,
                                   const float* poses, int64_t nf, int h, int w, const double* cam_inv_host,
                                   const double* bounds, double* keys, float* image_xyz, uint8_t* image_mask,
                                   float* images_out, int32_t* num_valid, void* stream) {
  MVK_REQUIRE(G >= 0 && nv >= 0 && nf >= 0 && h >= 0 && w >= 0, "chunk_unproject: bad sizes G=%d nv=%d nf=%lld h=%d w=%d", G,
              nv, (long long)nf, h, w);
  const int64_t hw = (int64_t)h * w, P = (int64_t)nv * hw;
  const int64_t bpc = cdiv64(P, UP_T);
  MVK_REQUIRE(nf < MAX_SIZE && P < MAX_SIZE && (hw == 0 || nf < MAX_SIZE / hw / 3) && (P == 0 || G < MAX_SIZE / P / 3) &&
                  (int64_t)G * bpc <= MAX_GRID,
              "chunk_unproject: sizes of 2^31 or more (G=%d nv=%d nf=%lld h=%d w=%d)", G, nv, (long long)nf, h, w);
  if (G == 0) return 0;
  MVK_REQUIRE(num_valid, "chunk_unproject: null operand");
  hipStream_t st = (hipStream_t)stream;
  MVK_CHECK_HIP(hipMemsetAsync(num_valid, 0, (size_t)G * sizeof(int32_t), st));
  if (P == 0) return 0;
  MVK_REQUIRE(sel && depth && images_in && poses && cam_inv_host && bounds && keys && image_xyz && image_mask && images_out,
              "chunk_unproject: null operand");
  Cam cam;
  for (int i = 0; i < 9; ++i) cam.kinv[i] = cam_inv_host[i];          // HOST pointer: 9 doubles
  hipLaunchKernelGGL(chunk_unproject_k, dim3((unsigned)(G * bpc)), dim3(UP_T), 0, st, sel, nv, depth, images_in, poses,
                     (int)nf, h, w, (int)bpc, cam, bounds, keys, image_xyz, image_mask, images_out, num_valid);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t mvk_scene_inputs_workspace(const int64_t* row_len_host, int G, int64_t nk, int k) {
  int64_t bytes = 256;
  for (int g = 0; row_len_host && g < G; ++g) {
    const int64_t b = mvk_knn_workspace(row_len_host[g] > 0 ? row_len_host[g] : 0, nk, k);
    if (b > bytes) bytes = b;
  }
  return bytes;
}

extern "C" int mvk_chunk_knn_many(const float* points, int64_t N, const int64_t* rows, int64_t total,
                                  const int64_t* row_off, const int64_t* q_off, const int64_t* row_len_host,
                                  const int64_t* q_off_host, int G, const double* keys, const uint8_t* key_valid,
                                  int64_t nk, int k, float* queries, int64_t* knn, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  MVK_REQUIRE(N >= 0 && total >= 0 && G >= 0 && nk >= 0 && N < MAX_SIZE && total < MAX_SIZE && nk < MAX_SIZE &&
                  (nk == 0 || G < MAX_SIZE / nk),
              "chunk_knn_many: bad sizes N=%lld total=%lld G=%d nk=%lld", (long long)N, (long long)total, G, (long long)nk);
  MVK_REQUIRE(k >= 1 && k <= 8, "chunk_knn_many: k=%d unsupported (1..8)", k);
  if (G == 0) return 0;
  MVK_REQUIRE(row_len_host && q_off_host, "chunk_knn_many: null host operand");
  MVK_REQUIRE(q_off_host[0] == 0, "chunk_knn_many: q_off_host must start at 0");
  for (int g = 0; g < G; ++g)
    MVK_REQUIRE(row_len_host[g] >= 0 && q_off_host[g + 1] == q_off_host[g] + row_len_host[g] && q_off_host[g + 1] < MAX_SIZE,
                "chunk_knn_many: q_off_host is not the running sum of row_len_host at chunk %d, or reaches 2^31", g);
  const int64_t sum = q_off_host[G];
  if (sum == 0) return 0;
  MVK_REQUIRE(rows && row_off && q_off && queries && knn && (points || N == 0) && (keys || nk == 0) &&
                  (key_valid || nk == 0),
              "chunk_knn_many: null operand");
  MVK_REQUIRE(workspace && workspace_bytes >= mvk_scene_inputs_workspace(row_len_host, G, nk, k),
              "chunk_knn_many: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(chunk_queries_k, dim3((unsigned)cdiv64(sum, BR_T)), dim3(BR_T), 0, st, points, N, rows, total, row_off,
                     q_off, G, sum, queries);
  MVK_CHECK_HIP(hipGetLastError());
  // the calls follow each other in stream order and read nothing back: one workspace serves them all
  for (int g = 0; g < G; ++g) {
    const int rc = mvk_knn_f64(queries + q_off_host[g] * 3, row_len_host[g], keys + (int64_t)g * nk * 3,
                               key_valid + (int64_t)g * nk, nk, k, knn + q_off_host[g] * k, workspace, workspace_bytes, st);
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" int mvk_chunk_batch_rows(const float* queries, const int64_t* knn, const int64_t* q_off, const int64_t* row_len,
                                    const int64_t* lengths, const int32_t* extras, const int64_t* extra_off, int G,
                                    int64_t n_max, int k, float* points_out, int64_t* knn_out, void* stream) {
  MVK_REQUIRE(G >= 0 && n_max >= 0 && k >= 0 && n_max < MAX_SIZE, "chunk_batch_rows: bad sizes G=%d n_max=%lld k=%d", G,
              (long long)n_max, k);
  const int64_t bpc = cdiv64(n_max, BR_T);
  MVK_REQUIRE((n_max == 0 || (int64_t)G * (k > 3 ? k : 3) < MAX_SIZE / n_max) && (int64_t)G * bpc <= MAX_GRID,
              "chunk_batch_rows: sizes of 2^31 or more (G=%d n_max=%lld k=%d)", G, (long long)n_max, k);
  if (G == 0 || n_max == 0) return 0;
  MVK_REQUIRE(queries && q_off && row_len && lengths && extra_off && points_out && (k == 0 || (knn && knn_out)),
              "chunk_batch_rows: null operand");
  hipLaunchKernelGGL(chunk_batch_rows_k, dim3((unsigned)(G * bpc)), dim3(BR_T), 0, (hipStream_t)stream, queries, knn, q_off,
                     row_len, lengths, extras, extra_off, (int)bpc, n_max, k, points_out, knn_out);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
