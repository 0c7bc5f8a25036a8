// Multi-view 2D -> 3D fusion inputs on gfx950:
//   * depth back-projection   (reference KPConv-PyTorch/datasets/ScanNet_sphere_color.py:66-72, :409-417)
//   * exact k-NN of sphere points among the unprojected pixels, float64, brute force with the keys
//     tiled through LDS (reference: scikit-learn NearestNeighbors(ball_tree), :448-451)
//   * group_points gather / scatter-add (reference mvpnet/ops/cuda/group_points_kernel.cu:25-145)
// Compiled with -ffp-contract=off: the float64 products and sums are evaluated exactly in the
// written order, like the NumPy / scikit-learn code they replace.
#include "common.h"
#include "compact.h"
#include "knn_core.h"
#include "ball.h"
#include "unproject.h"

namespace {

// ---------------------------------------------------------------------------------------------
// xyz_cam = (Kinv . [u, v, 1]) * depth ;  valid = z_cam > 0 ;  xyz_world = xyz_cam . R^T + t  (unproject.h)
// ---------------------------------------------------------------------------------------------
__global__ void unproject_kernel(const uint16_t* __restrict__ depth, int nv, int h, int w, Cam cam,
                                 const float* __restrict__ poses, double* __restrict__ xyz,
                                 uint8_t* __restrict__ valid) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t hw = (int64_t)h * w;
  if (t >= nv * hw) return;
  const int view = (int)(t / hw);
  const int pix = (int)(t % hw);
  const double u = (double)(pix % w), v = (double)(pix / w);
  double c[3], x[3];
  unproject_pixel(cam, poses + view * 16, u, v, depth[t], c, x);
  valid[t] = c[2] > 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) xyz[t * 3 + r] = x[r];
}

// ---------------------------------------------------------------------------------------------
// brute-force k-NN, float64. One lane = one query; a 256-lane workgroup stages 256 keys at a time
// in LDS (coalesced loads, broadcast reads); top-k kept sorted in registers (k <= 8).
// Keys are split into `nsplit` contiguous ranges (grid.y) so that small query sets still fill the
// chip; a merge kernel combines the per-split candidates.
// ---------------------------------------------------------------------------------------------
constexpr int KNN_T = 256;
constexpr int KMAXNN = 8;

// QPT queries per lane: every LDS key read (3 broadcast ds_read_b64) is reused QPT times, which moves the
// loop from LDS-issue bound (1 query per lane: ~6 LDS cycles per 28 fp64 VALU cycles per wave, four waves
// sharing one LDS) to fp64-VALU bound.
constexpr int QPT = 4;

template <int K>
__global__ __launch_bounds__(KNN_T) void knn_partial_kernel(const float* __restrict__ q, int64_t nq,
                                                            const double* __restrict__ keys,
                                                            const uint8_t* __restrict__ kvalid,
                                                            int64_t nk, int64_t per_split,
                                                            double* __restrict__ pd,
                                                            int64_t* __restrict__ pi) {
  __shared__ double kx[KNN_T], ky[KNN_T], kz[KNN_T];
  __shared__ int kok[KNN_T];
  const int64_t i0 = ((int64_t)blockIdx.x * KNN_T + threadIdx.x) * QPT;
  const int64_t kbeg = (int64_t)blockIdx.y * per_split, kend = min(nk, kbeg + per_split);
  double qx[QPT], qy[QPT], qz[QPT];
  double bd[QPT][K];
  int64_t bi[QPT][K];
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const int64_t i = i0 + u;
    qx[u] = i < nq ? (double)q[i * 3] : 0.0;
    qy[u] = i < nq ? (double)q[i * 3 + 1] : 0.0;
    qz[u] = i < nq ? (double)q[i * 3 + 2] : 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      bd[u][c] = INFINITY;
      bi[u][c] = INT64_MAX;
    }
  }
  for (int64_t k0 = kbeg; k0 < kend; k0 += KNN_T) {
    const int64_t j = k0 + threadIdx.x;
    if (j < kend) {
      kx[threadIdx.x] = keys[j * 3];
      ky[threadIdx.x] = keys[j * 3 + 1];
      kz[threadIdx.x] = keys[j * 3 + 2];
      kok[threadIdx.x] = kvalid ? (int)kvalid[j] : 1;
    } else {
      kok[threadIdx.x] = 0;
    }
    __syncthreads();
    const int cnt = (int)min((int64_t)KNN_T, kend - k0);
    for (int t = 0; t < cnt; ++t) {
      if (!kok[t]) continue;  // uniform across the workgroup
      const double x = kx[t], y = ky[t], z = kz[t];
#pragma unroll
      for (int u = 0; u < QPT; ++u) {
        topk_insert<K>(bd[u], bi[u], knn_d2(qx[u], qy[u], qz[u], x, y, z), k0 + t);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    const int64_t i = i0 + u;
    if (i < nq) {
#pragma unroll
      for (int c = 0; c < K; ++c) {
        pd[((int64_t)blockIdx.y * nq + i) * K + c] = bd[u][c];
        pi[((int64_t)blockIdx.y * nq + i) * K + c] = bi[u][c];
      }
    }
  }
}

template <int K>
__global__ void knn_merge_kernel(const double* __restrict__ pd, const int64_t* __restrict__ pi, int nsplit,
                                 int64_t nq, int kout, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  double bd[K];
  int64_t bi[K];
#pragma unroll
  for (int c = 0; c < K; ++c) {
    bd[c] = INFINITY;
    bi[c] = INT64_MAX;
  }
  for (int s = 0; s < nsplit; ++s)
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const double d = pd[((int64_t)s * nq + i) * K + c];
      const int64_t j = pi[((int64_t)s * nq + i) * K + c];
      if (j != INT64_MAX) topk_insert<K>(bd, bi, d, j);
    }
#pragma unroll
  for (int c = 0; c < K; ++c)
    if (c < kout) out[i * kout + c] = bi[c] == INT64_MAX ? -1 : bi[c];
}

// ---------------------------------------------------------------------------------------------
// Pruned exact k-NN (same results as the brute-force kernels above, bit for bit): the Morton grid, the tile boxes and
// the search of one workgroup are csrc/knn_core.h's, shared with mvk_knn_f64_ragged. Here: one key set, sized by the host.
// ---------------------------------------------------------------------------------------------
struct PrunedWs {
  int* cnt;        // [2][PNC]   (0 = queries, 1 = keys), zeroed by the host
  int* start;      // [2][PNC]
  int* cell;       // [nq + nk]
  int* rank;       // [nq + nk]
  int* qorder;     // [nq]
  double* skey;    // [nk][3] sorted valid keys
  int* sidx;       // [nk]    their original index
  float* box;      // [ntiles_max][8]  lo xyz, hi xyz, count, pad
  int* nvalid;     // [1]
};

// One counter update per wavefront and distinct cell, not per element: neighbouring pixels unproject into the same 10 cm
// cell (a cell close to a camera holds thousands of keys), and returning atomics on one address retire one after the other
// -- with an atomic per key the hottest cell set the kernel's time (177 us for 96 000 keys of five views, 25 us for three
// views). The lanes of a wavefront are grouped by cell with ballots first (no memory traffic), then every group's first
// lane adds the group's size once and the others take their rank from its return value.
__global__ __launch_bounds__(256) void pk_count_kernel(const float* __restrict__ q, int64_t nq, const double* __restrict__ keys,
                                                       const uint8_t* __restrict__ kvalid, int64_t nk, PrunedWs ws) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool valid = e < nq + nk;
  int key = -1;                                  // set * PNC + cell
  if (valid) {
    if (e < nq) {
      key = morton_cell(q[e * 3], q[e * 3 + 1], q[e * 3 + 2]);
    } else {
      const int64_t j = e - nq;
      if (kvalid && !kvalid[j]) {
        ws.cell[e] = -1;
        valid = false;
      } else {
        key = PNC + morton_cell((float)keys[j * 3], (float)keys[j * 3 + 1], (float)keys[j * 3 + 2]);
      }
    }
  }
  int leader = lane, before = 0, group = 1;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int first = __ffsll((long long)todo) - 1;
    const int k0 = __shfl(key, first);
    const bool mine = valid && key == k0;
    const unsigned long long same = __ballot(mine);
    if (mine) {
      leader = first;
      before = __popcll(same & ((1ull << lane) - 1ull));
      group = __popcll(same);
    }
    todo &= ~same;
  }
  int base = 0;
  if (valid && leader == lane) base = atomicAdd(ws.cnt + key, group);
  base = __shfl(base, leader);
  if (valid) {
    ws.cell[e] = key >= PNC ? key - PNC : key;
    ws.rank[e] = base + before;
  }
}

// exclusive scan of the PNC cell counts of one set (blockIdx.x), 1024 threads x 32 cells
__global__ __launch_bounds__(1024) void pk_scan_kernel(PrunedWs ws) {
  const int set = blockIdx.x;
  const int total = pk_scan_cells(ws.cnt + set * PNC, ws.start + set * PNC);
  if (set == 1 && threadIdx.x == 1023) *ws.nvalid = total;
}

__global__ void pk_scatter_kernel(int64_t nq, const double* __restrict__ keys, int64_t nk, PrunedWs ws) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nq + nk) return;
  const int c = ws.cell[e];
  if (c < 0) return;
  if (e < nq) {
    ws.qorder[ws.start[c] + ws.rank[e]] = (int)e;
  } else {
    const int64_t j = e - nq;
    const int p = ws.start[PNC + c] + ws.rank[e];
    ws.skey[(int64_t)p * 3] = keys[j * 3];
    ws.skey[(int64_t)p * 3 + 1] = keys[j * 3 + 1];
    ws.skey[(int64_t)p * 3 + 2] = keys[j * 3 + 2];
    ws.sidx[p] = (int)j;
  }
}

// one wave per tile: outward-rounded float box of its keys
__global__ __launch_bounds__(64) void pk_box_kernel(PrunedWs ws) {
  pk_tile_box(ws.skey, *ws.nvalid, blockIdx.x, ws.box + (int64_t)blockIdx.x * 8);
}

template <int K, int PW>   // PW waves per workgroup share one set of 64 queries
__global__ __launch_bounds__(64 * PW) void knn_pruned_kernel(const float* __restrict__ q, int64_t nq, PrunedWs ws,
                                                             int ntiles_max, int kout,
                                                             int64_t* __restrict__ out) {
  const int64_t slot = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const bool live = slot < nq;
  knn_pruned_search<K, PW>(q, live, live ? ws.qorder[slot] : 0, ws.box, ws.skey, ws.sidx, *ws.nvalid, ntiles_max, kout, out);
}

// ---------------------------------------------------------------------------------------------
// group_points: out[b,c,n,k] = in[b,c,idx[b,n,k]]; one lane per output element, (n,k) fastest so
// index reads and output writes are coalesced; the gather itself is element granular by nature
// (channel-major feature maps), served by L2 / Infinity Cache.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void group_points_fwd_kernel(const T* __restrict__ in, const int64_t* __restrict__ idx, int B,
                                        int C, int64_t N1, int64_t NK, T* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * C * NK) return;
  const int64_t e = t % NK;
  const int64_t bc = t / NK;
  const int64_t b = bc / C;
  const int64_t j = idx[b * NK + e];
  out[t] = (j >= 0 && j < N1) ? in[bc * N1 + j] : (T)0;
}

template <typename T>
__global__ void group_points_bwd_kernel(const T* __restrict__ go, const int64_t* __restrict__ idx, int B,
                                        int C, int64_t N1, int64_t NK, T* __restrict__ gi) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * C * NK) return;
  const int64_t e = t % NK;
  const int64_t bc = t / NK;
  const int64_t b = bc / C;
  const int64_t j = idx[b * NK + e];
  if (j >= 0 && j < N1) atomicAdd(gi + bc * N1 + j, go[t]);  // group_points_kernel.cu:85-87
}

// ---------------------------------------------------------------------------------------------
// Fused input of FeatureAggregation (reference mvpnet/models/mvpnet_3d.py:54-58 fed by the two
// group_points calls of architectures_sphere.py:266-274): for every (point n, neighbour kk) pair
//   X[c, n*k+kk]   = feature_2d[view(p), c, pix(p)]            c < C,  p = knn[n,kk]
//   X[C+0..2, .]   = image_xyz[p] - point[n]                   (diff_xyz)
//   X[C+3, .]      = |diff|^2                                   (sum of squares in x,y,z order)
// X is channel-major [C+4, np*k] (the layout the 1x1 convolution wants as a transposed GEMM operand);
// lanes run over pairs, so every channel row is written coalesced and the gather stays inside one
// h*w channel plane (L2 resident). Reads the 2D feature map in its native (nv, C, h, w) layout: the
// (b, C, nv*h*w) transpose copy of the reference is not needed.
// ---------------------------------------------------------------------------------------------
__global__ void fa_gather_kernel(const float* __restrict__ feat /* [nv,C,hw], or [nv,hw,C] (channels last) */,
                                 const float* __restrict__ xyz /* [nv*hw,3] */,
                                 const int64_t* __restrict__ knn /* [np*k] */, const float* __restrict__ pts /* [np,3] */,
                                 int C, int nv, int64_t hw, int64_t npk, int k, float* __restrict__ X /* [C+4, npk] */,
                                 int64_t ch_stride, int64_t px_stride) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= npk) return;
  const int64_t p = knn[e];
  const bool ok = p >= 0 && p < nv * hw;
  const int64_t view = ok ? p / hw : 0, pix = ok ? p % hw : 0;
  const float* f = feat + view * C * hw + pix * px_stride;
  for (int c = blockIdx.y; c < C; c += gridDim.y) X[(int64_t)c * npk + e] = ok ? f[(int64_t)c * ch_stride] : 0.f;
  if (blockIdx.y == 0) {
    const int64_t n = e / k;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (ok) {
      dx = xyz[p * 3] - pts[n * 3];
      dy = xyz[p * 3 + 1] - pts[n * 3 + 1];
      dz = xyz[p * 3 + 2] - pts[n * 3 + 2];
    }
    X[(int64_t)C * npk + e] = dx;
    X[(int64_t)(C + 1) * npk + e] = dy;
    X[(int64_t)(C + 2) * npk + e] = dz;
    X[(int64_t)(C + 3) * npk + e] = (dx * dx + dy * dy) + dz * dz;
  }
}

// ---------------------------------------------------------------------------------------------
// Sphere extraction around a centre (reference ScanNetDataset.potential_item,
// KPConv-PyTorch/datasets/ScanNet_sphere_color.py:556-597: sklearn KDTree.query_radius on float64
// data, membership rdist = dx^2+dy^2+dz^2 <= r^2) and the Tukey update of the sampling potentials
// (:576-584). Points are float32 promoted to float64 like the tree's data; evaluation order as
// sklearn's euclidean rdist. Ordered stream compaction: per-block ballot counts -> block scan ->
// scatter, so the indices come out ascending (the reference's order is KD-tree traversal order; the
// contract here is the SET).
// ---------------------------------------------------------------------------------------------
// grid ceil(N/1024), block 1024: block_count[b] = members in the block
__global__ __launch_bounds__(1024) void ball_count_kernel(const float* __restrict__ pts, int64_t N, Ball b,
                                                          int* __restrict__ block_count) {
  __shared__ int wc[16];
  const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  const bool in = i < N && ball_rdist(pts, i, b) <= b.r2;
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < 16; ++w) t += wc[w];
    block_count[blockIdx.x] = t;
  }
}

// single block: exclusive scan of block counts in place, total -> *count
__global__ __launch_bounds__(1024) void ball_scan_kernel(int* __restrict__ block_count, int nblk, int64_t* __restrict__ count) {
  __shared__ int carry;
  __shared__ int ws[16];
  const int total = compact_scan_counts(block_count, nblk, &carry, ws);
  if (threadIdx.x == 0) *count = total;
}

__global__ __launch_bounds__(1024) void ball_scatter_kernel(const float* __restrict__ pts, int64_t N, Ball b,
                                                            const int* __restrict__ block_off,
                                                            int64_t* __restrict__ out_idx, double* __restrict__ out_d2) {
  __shared__ int wc[16];
  const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  double d2 = 0.0;
  bool in = false;
  if (i < N) {
    d2 = ball_rdist(pts, i, b);
    in = d2 <= b.r2;
  }
  const unsigned long long m = __ballot(in);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wc[w] = __popcll(m);
  __syncthreads();
  if (in) {
    const int off = block_off[blockIdx.x] + compact_wave_offset(wc, w) + compact_lane_rank(m);
    out_idx[off] = i;
    if (out_d2) out_d2[off] = d2;
  }
}

// potentials[i] += tukey(d2) for the members (ScanNet_sphere_color.py:576-582)
__global__ void tukey_update_kernel(const float* __restrict__ pts, int64_t N, Ball b, double* __restrict__ pot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double rd = ball_rdist(pts, i, b);
  if (rd <= b.r2) {
    pot[i] += tukey_weight(rd, b.r2);
  }
}

}  // namespace

extern "C" int64_t mvk_ball_query_workspace(int64_t N) { return (cdiv64(N > 0 ? N : 1, 1024) + 4) * 4 + 64; }

extern "C" int mvk_ball_query(const float* pts, int64_t N, const double* center_host, double radius,
                              int64_t* out_idx, double* out_d2, int64_t* count_dev, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  MVK_REQUIRE(N >= 0 && radius >= 0.0, "ball_query: bad arguments");
  MVK_REQUIRE(workspace && workspace_bytes >= mvk_ball_query_workspace(N), "ball_query: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)cdiv64(N > 0 ? N : 1, 1024);
  Ball b{center_host[0], center_host[1], center_host[2], radius * radius};
  int* bc = (int*)workspace;
  hipLaunchKernelGGL(ball_count_kernel, dim3(nblk), dim3(1024), 0, st, pts, N, b, bc);
  hipLaunchKernelGGL(ball_scan_kernel, dim3(1), dim3(1024), 0, st, bc, nblk, count_dev);
  hipLaunchKernelGGL(ball_scatter_kernel, dim3(nblk), dim3(1024), 0, st, pts, N, b, bc, out_idx, out_d2);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_tukey_update(const float* pts, int64_t N, const double* center_host, double radius,
                                double* potentials, void* stream) {
  MVK_REQUIRE(N >= 0 && radius > 0.0, "tukey_update: bad arguments");
  if (N == 0) return 0;
  Ball b{center_host[0], center_host[1], center_host[2], radius * radius};
  hipLaunchKernelGGL(tukey_update_kernel, dim3((unsigned)cdiv64(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, N, b,
                     potentials);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

namespace {

}  // namespace

extern "C" int mvk_fa_gather_fwd_ex(const float* feature_2d, int channels_last, const float* image_xyz, const int64_t* knn,
                                    const float* points, int C, int nv, int64_t hw, int64_t np, int k, float* X,
                                    void* stream) {
  MVK_REQUIRE(C > 0 && nv > 0 && hw > 0 && np >= 0 && k > 0, "fa_gather: bad sizes");
  const int64_t npk = np * k;
  if (npk == 0) return 0;
  // channels last: a pixel's C channels are one contiguous run, the 8 channel slices of a point (grid.y) share its lines
  dim3 grid((unsigned)cdiv64(npk, 256), 8);
  hipLaunchKernelGGL(fa_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, feature_2d, image_xyz, knn, points, C, nv,
                     hw, npk, k, X, channels_last ? (int64_t)1 : hw, channels_last ? (int64_t)C : (int64_t)1);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_fa_gather_fwd(const float* feature_2d, const float* image_xyz, const int64_t* knn,
                                 const float* points, int C, int nv, int64_t hw, int64_t np, int k, float* X,
                                 void* stream) {
  return mvk_fa_gather_fwd_ex(feature_2d, 0, image_xyz, knn, points, C, nv, hw, np, k, X, stream);
}

extern "C" int mvk_unproject_depth(const uint16_t* depth, int nv, int h, int w, const double* cam_inv,
                                   const float* poses, double* xyz, uint8_t* valid, void* stream) {
  MVK_REQUIRE(nv >= 0 && h > 0 && w > 0, "unproject: bad sizes");
  if (nv == 0) return 0;
  Cam cam;
  for (int i = 0; i < 9; ++i) cam.kinv[i] = cam_inv[i];  // HOST pointer: 9 doubles
  const int64_t tot = (int64_t)nv * h * w;
  hipLaunchKernelGGL(unproject_kernel, dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream, depth,
                     nv, h, w, cam, poses, xyz, valid);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

namespace {
// key splits: enough (query block x key range) workgroups to give every CU ~4 of them
void knn_plan(int64_t nq, int64_t nk, int* nsplit_out, int64_t* per_split_out) {
  const int64_t qblocks = cdiv64(nq > 0 ? nq : 1, KNN_T * QPT);
  const int64_t keys = nk > 0 ? nk : 1;
  int64_t nsplit = cdiv64(1024, qblocks);
  const int64_t max_split = cdiv64(keys, 4 * KNN_T);
  if (nsplit > max_split) nsplit = max_split;
  if (nsplit < 1) nsplit = 1;
  if (nsplit > 64) nsplit = 64;
  const int64_t per_split = cdiv64(cdiv64(keys, nsplit), KNN_T) * KNN_T;
  *nsplit_out = (int)cdiv64(keys, per_split);
  *per_split_out = per_split;
}
}  // namespace

namespace {
int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// the pruned path pays five small launches: only worth it when the brute-force product is large
bool knn_use_pruned(int64_t nq, int64_t nk) {
  const char* e = getenv("MVK_KNN_BRUTE");
  if (e && e[0] == '1') return false;
  return nq >= 1024 && nk >= 4096 && nq + nk < (int64_t)1 << 30;
}

int64_t pruned_layout(int64_t nq, int64_t nk, char* base, PrunedWs* ws) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  const int64_t ntiles = cdiv64(nk, PT);
  char* cnt = take(2 * PNC * 4);
  char* start = take(2 * PNC * 4);
  char* cell = take((nq + nk) * 4);
  char* rank = take((nq + nk) * 4);
  char* qorder = take(nq * 4);
  char* skey = take(nk * 24);
  char* sidx = take(nk * 4);
  char* box = take(ntiles * 32);
  char* nvalid = take(4);
  if (ws) {
    ws->cnt = (int*)cnt; ws->start = (int*)start; ws->cell = (int*)cell; ws->rank = (int*)rank;
    ws->qorder = (int*)qorder; ws->skey = (double*)skey; ws->sidx = (int*)sidx; ws->box = (float*)box;
    ws->nvalid = (int*)nvalid;
  }
  return off;
}
}  // namespace

extern "C" int64_t mvk_knn_workspace(int64_t nq, int64_t nk, int k) {
  int nsplit;
  int64_t per;
  knn_plan(nq, nk, &nsplit, &per);
  const int64_t brute = (int64_t)nsplit * (nq > 0 ? nq : 1) * (k <= 3 ? 3 : 8) * 16 + 64;
  const int64_t pruned = pruned_layout(nq > 0 ? nq : 1, nk > 0 ? nk : 1, nullptr, nullptr) + 256;
  return brute > pruned ? brute : pruned;
}

extern "C" int mvk_knn_f64(const float* queries, int64_t nq, const double* keys, const uint8_t* key_valid,
                           int64_t nk, int k, int64_t* out_idx, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  MVK_REQUIRE(k >= 1 && k <= KMAXNN, "knn: k=%d unsupported (1..%d)", k, KMAXNN);
  MVK_REQUIRE(nq >= 0 && nk >= 0, "knn: bad sizes");
  if (nq == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int nsplit;
  int64_t per_split;
  knn_plan(nq, nk, &nsplit, &per_split);
  const int KK = k <= 3 ? 3 : 8;
  MVK_REQUIRE(workspace && workspace_bytes >= mvk_knn_workspace(nq, nk, k), "knn: workspace too small");
  if (knn_use_pruned(nq, nk)) {
    PrunedWs ws;
    char* base = (char*)(((uintptr_t)workspace + 255) / 256 * 256);
    pruned_layout(nq, nk, base, &ws);
    const int ntiles = (int)cdiv64(nk, PT);
    MVK_CHECK_HIP(hipMemsetAsync(ws.cnt, 0, 2 * PNC * 4, st));
    const unsigned eb = (unsigned)cdiv64(nq + nk, 256);
    hipLaunchKernelGGL(pk_count_kernel, dim3(eb), dim3(256), 0, st, queries, nq, keys, key_valid, nk, ws);
    hipLaunchKernelGGL(pk_scan_kernel, dim3(2), dim3(1024), 0, st, ws);
    hipLaunchKernelGGL(pk_scatter_kernel, dim3(eb), dim3(256), 0, st, nq, keys, nk, ws);
    hipLaunchKernelGGL(pk_box_kernel, dim3((unsigned)ntiles), dim3(64), 0, st, ws);
    const dim3 grid((unsigned)cdiv64(nq, 64));
    if (KK == 3)
      hipLaunchKernelGGL((knn_pruned_kernel<3, 8>), grid, dim3(64 * 8), 0, st, queries, nq, ws, ntiles, k, out_idx);
    else
      hipLaunchKernelGGL((knn_pruned_kernel<8, 4>), grid, dim3(64 * 4), 0, st, queries, nq, ws, ntiles, k, out_idx);
    MVK_CHECK_HIP(hipGetLastError());
    return 0;
  }
  double* pd = (double*)workspace;
  int64_t* pi = (int64_t*)((char*)workspace + (int64_t)nsplit * nq * KK * 8);
  dim3 grid((unsigned)cdiv64(nq, KNN_T * QPT), (unsigned)nsplit);
  if (KK == 3) {
    hipLaunchKernelGGL((knn_partial_kernel<3>), grid, dim3(KNN_T), 0, st, queries, nq, keys, key_valid, nk,
                       per_split, pd, pi);
    hipLaunchKernelGGL((knn_merge_kernel<3>), dim3((unsigned)cdiv64(nq, 256)), dim3(256), 0, st, pd, pi, nsplit,
                       nq, k, out_idx);
  } else {
    hipLaunchKernelGGL((knn_partial_kernel<8>), grid, dim3(KNN_T), 0, st, queries, nq, keys, key_valid, nk,
                       per_split, pd, pi);
    hipLaunchKernelGGL((knn_merge_kernel<8>), dim3((unsigned)cdiv64(nq, 256)), dim3(256), 0, st, pd, pi, nsplit,
                       nq, k, out_idx);
  }
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_group_points_fwd(const float* points, const int64_t* index, int B, int C, int64_t N1,
                                    int64_t N2, int K, float* out, void* stream) {
  MVK_REQUIRE(B >= 0 && C >= 0 && N1 >= 0 && N2 >= 0 && K >= 0, "group_points: bad sizes");
  const int64_t tot = (int64_t)B * C * N2 * K;
  if (tot == 0) return 0;
  hipLaunchKernelGGL(group_points_fwd_kernel<float>, dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream,
                     points, index, B, C, N1, N2 * K, out);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

// float64 twins (the reference's extension dispatches float and double, group_points_kernel.cu:60,130)
extern "C" int mvk_group_points_fwd_f64(const double* points, const int64_t* index, int B, int C, int64_t N1,
                                        int64_t N2, int K, double* out, void* stream) {
  MVK_REQUIRE(B >= 0 && C >= 0 && N1 >= 0 && N2 >= 0 && K >= 0, "group_points: bad sizes");
  const int64_t tot = (int64_t)B * C * N2 * K;
  if (tot == 0) return 0;
  hipLaunchKernelGGL(group_points_fwd_kernel<double>, dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream,
                     points, index, B, C, N1, N2 * K, out);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_group_points_bwd_f64(const double* grad_out, const int64_t* index, int B, int C, int64_t N1,
                                        int64_t N2, int K, double* grad_in, void* stream) {
  const int64_t tot = (int64_t)B * C * N2 * K;
  if (tot == 0) return 0;
  hipLaunchKernelGGL(group_points_bwd_kernel<double>, dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream,
                     grad_out, index, B, C, N1, N2 * K, grad_in);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_group_points_bwd(const float* grad_out, const int64_t* index, int B, int C, int64_t N1,
                                    int64_t N2, int K, float* grad_in, void* stream) {
  const int64_t tot = (int64_t)B * C * N2 * K;
  if (tot == 0) return 0;
  hipLaunchKernelGGL(group_points_bwd_kernel<float>, dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream,
                     grad_out, index, B, C, N1, N2 * K, grad_in);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
