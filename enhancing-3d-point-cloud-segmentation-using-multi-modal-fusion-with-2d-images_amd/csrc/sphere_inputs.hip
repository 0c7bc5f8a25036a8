// Sphere batches of the KPFCNN networks on gfx950 from scenes resident in HBM (include/mvkpconv_sphere.h; reference:
// KPConv-PyTorch/datasets/ScanNet_sphere_color.py:494-720, potential_item, which is NumPy and scikit-learn trees in
// DataLoader workers). Every entry point has a fixed number of launches for B_max sphere slots; nothing is read back.
//   mvk_knn_f64_ragged      the exact float64 k-NN of B items whose lengths exist only on the device: the pruned search of
//                           mvk_knn_f64 (csrc/fusion.hip) with an item dimension. The arithmetic and the search of one
//                           workgroup are csrc/knn_core.h's, shared with it, so the two give the same bits.
//   sphere_pick_k           one workgroup: arg-min of the potentials, Tukey update, new arg-min, sphere size, stop rule
//   sphere_members_k        compact.h's three steps over all slots: tile counts, scan (+ q_off), ordered scatter
//   sphere_select_frames_k  select_frames.h's greedy coverage on the slot's mask row
//   sphere_batch_rows_k     centred, augmented points, features, labels and stacked k-NN of every row
// The unprojection is mvk_train_unproject with a box no pixel can leave.
// Compiled with -ffp-contract=off: float32 / float64 products and sums are evaluated exactly in the written order.
#include "common.h"
#include "ball.h"
#include "compact.h"
#include "knn_core.h"
#include "resident.h"
#include "select_frames.h"
#include "../../include/mvkpconv_scene.h"
#include "../../include/mvkpconv_sphere.h"

namespace {

constexpr int RK_ITEM_SHIFT = 15;                 // cell word = Morton cell (15 bits) | item << 15
static_assert(PNC == 1 << RK_ITEM_SHIFT, "cell word layout");
static_assert(MVK_KNN_RAGGED_MAX_ITEMS == 1024, "rk_plan_kernel is one workgroup of 1024 threads");

struct RaggedWs {
  int* lo;         // [B+1]        q_off clamped to [0, cap] and made non-decreasing
  int* wg_off;     // [B+1]        first search workgroup of every item; [B] = their number
  int* cnt;        // [B][2][PNC]  (0 = queries, 1 = keys), zeroed by the host
  int* start;      // [B][2][PNC]
  int* cell;       // [cap + B*nk] cell word, -1 = takes no part
  int* rank;       // [cap + B*nk]
  int* qorder;     // [cap]        item b's sorted queries at lo[b] ..: their slots
  double* skey;    // [B][nk][3]   sorted valid keys
  int* sidx;       // [B][nk]      their number in the item
  float* box;      // [B][ntiles][8]
  int* nvalid;     // [B]
  float* qbuf;     // [cap][3]     the gathered queries (the caller's queries_out when it gives one)
};

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

int64_t ragged_layout(int B, int64_t cap, int64_t nk, bool own_queries, char* base, RaggedWs* ws) {
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  const int64_t ntiles = cdiv64(nk, PT), e = cap + (int64_t)B * nk;
  char* lo = take((B + 1) * 4);
  char* wg_off = take((B + 1) * 4);
  char* cnt = take((int64_t)B * 2 * PNC * 4);
  char* start = take((int64_t)B * 2 * PNC * 4);
  char* cell = take(e * 4);
  char* rank = take(e * 4);
  char* qorder = take(cap * 4);
  char* skey = take((int64_t)B * nk * 24);
  char* sidx = take((int64_t)B * nk * 4);
  char* box = take((int64_t)B * ntiles * 32);
  char* nvalid = take((int64_t)B * 4);
  char* qbuf = take(own_queries ? cap * 12 : 0);
  if (ws) {
    ws->lo = (int*)lo; ws->wg_off = (int*)wg_off; ws->cnt = (int*)cnt; ws->start = (int*)start; ws->cell = (int*)cell;
    ws->rank = (int*)rank; ws->qorder = (int*)qorder; ws->skey = (double*)skey; ws->sidx = (int*)sidx;
    ws->box = (float*)box; ws->nvalid = (int*)nvalid; ws->qbuf = (float*)qbuf;
  }
  return off;
}

// inclusive scan of a[0..1024) in LDS by 1024 threads; OP is max or +
template <bool SUM>
__device__ __forceinline__ void rk_scan1024(int* a) {
  const int t = threadIdx.x;
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = t >= off ? a[t - off] : (SUM ? 0 : INT_MIN);
    __syncthreads();
    a[t] = SUM ? a[t] + v : max(a[t], v);
    __syncthreads();
  }
}

// One workgroup: lo[b] = the running maximum of q_off clamped to [0, cap]; item b has lo[b+1] - lo[b] queries and
// ceil(that / 64) search workgroups, numbered from wg_off[b].
__global__ __launch_bounds__(1024) void rk_plan_kernel(const int64_t* __restrict__ q_off, int B, int cap, RaggedWs ws) {
  __shared__ int a[1025];
  const int t = threadIdx.x;
  auto rd = [&](int i) {
    const int64_t v = q_off[i];
    return (int)(v < 0 ? 0 : v > cap ? cap : v);
  };
  a[t] = t <= B ? rd(t) : cap;
  __syncthreads();
  rk_scan1024<false>(a);
  if (t == 1023) a[1024] = B == 1024 ? max(a[1023], rd(1024)) : cap;
  __syncthreads();
  const int lo = a[t], hi = a[t + 1];
  if (t <= B) ws.lo[t] = lo;
  if (t == 1023 && B == 1024) ws.lo[1024] = hi;
  const int n = t < B ? (hi - lo + 63) / 64 : 0;
  __syncthreads();
  a[t] = n;
  __syncthreads();
  rk_scan1024<true>(a);
  if (t <= B) ws.wg_off[t] = a[t] - n;
  if (t == 1023 && B == 1024) ws.wg_off[1024] = a[1023];
}

// the last b in [0, n] with v[b] <= x, -1 when there is none (v non-decreasing, n + 1 entries)
__device__ __forceinline__ int rk_find(const int* __restrict__ v, int n, int x) {
  int a = 0, b = n + 1;          // the first entry > x lies in [a, b]
  while (a < b) {
    const int m = (a + b) >> 1;
    if (v[m] <= x) a = m + 1; else b = m;
  }
  return a - 1;
}

// Element e < cap is query slot e, element cap + b * nk + j is key j of item b. Gathers the query, bins both into their
// item's grid and counts per (item, set, cell) -- one counter update per wavefront and distinct cell, as
// pk_count_kernel of fusion.hip does and for its reason. Slots of no item get their -1 / zeros here.
__global__ __launch_bounds__(256) void rk_count_kernel(const float* __restrict__ points, int64_t N,
                                                       const int64_t* __restrict__ rows, int cap, int B,
                                                       const double* __restrict__ keys,
                                                       const uint8_t* __restrict__ kvalid, int nk, int k,
                                                       int64_t* __restrict__ knn, RaggedWs ws) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool valid = e < (int64_t)cap + (int64_t)B * nk;
  int key = -1, item = 0;                          // key = (item * 2 + set) * PNC + cell
  if (valid) {
    if (e < cap) {
      item = rk_find(ws.lo, B, (int)e);
      float x = 0.f, y = 0.f, z = 0.f;
      if (item < 0 || item >= B) {
        ws.cell[e] = -1;
        valid = false;
        for (int c = 0; c < k; ++c) knn[e * k + c] = -1;
      } else {
        const int64_t r = rows[e];
        if (r >= 0 && r < N) {
          x = points[r * 3];
          y = points[r * 3 + 1];
          z = points[r * 3 + 2];
        }
        key = item * 2 * PNC + morton_cell(x, y, z);
      }
      ws.qbuf[e * 3] = x;
      ws.qbuf[e * 3 + 1] = y;
      ws.qbuf[e * 3 + 2] = z;
    } else {
      const int64_t j = e - cap;
      item = (int)(j / nk);
      if (kvalid && !kvalid[j]) {
        ws.cell[e] = -1;
        valid = false;
      } else {
        key = (item * 2 + 1) * PNC + morton_cell((float)keys[j * 3], (float)keys[j * 3 + 1], (float)keys[j * 3 + 2]);
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
    ws.cell[e] = (key & (PNC - 1)) | (item << RK_ITEM_SHIFT);
    ws.rank[e] = base + before;
  }
}

// two workgroups per item: blockIdx.x = item * 2 + set
__global__ __launch_bounds__(1024) void rk_scan_kernel(RaggedWs ws) {
  const int total = pk_scan_cells(ws.cnt + (int64_t)blockIdx.x * PNC, ws.start + (int64_t)blockIdx.x * PNC);
  if ((blockIdx.x & 1) && threadIdx.x == 1023) ws.nvalid[blockIdx.x >> 1] = total;
}

// Item b holds exactly lo[b+1] - lo[b] queries and at most nk valid keys, so start + rank stays inside the item's part.
__global__ __launch_bounds__(256) void rk_scatter_kernel(int cap, int B, const double* __restrict__ keys, int nk,
                                                         RaggedWs ws) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)cap + (int64_t)B * nk) return;
  const int w = ws.cell[e];
  if (w < 0) return;
  const int item = w >> RK_ITEM_SHIFT, c = w & (PNC - 1);
  if (e < cap) {
    ws.qorder[ws.lo[item] + ws.start[(int64_t)item * 2 * PNC + c] + ws.rank[e]] = (int)e;
  } else {
    const int64_t j = e - cap;
    const int64_t p = (int64_t)item * nk + ws.start[((int64_t)item * 2 + 1) * PNC + c] + ws.rank[e];
    ws.skey[p * 3] = keys[j * 3];
    ws.skey[p * 3 + 1] = keys[j * 3 + 1];
    ws.skey[p * 3 + 2] = keys[j * 3 + 2];
    ws.sidx[p] = (int)(j - (int64_t)item * nk);
  }
}

// one wave per (tile, item)
__global__ __launch_bounds__(64) void rk_box_kernel(int nk, int ntiles, RaggedWs ws) {
  const int item = blockIdx.y;
  pk_tile_box(ws.skey + (int64_t)item * nk * 3, ws.nvalid[item], blockIdx.x,
              ws.box + ((int64_t)item * ntiles + blockIdx.x) * 8);
}

// Workgroup g searches 64 consecutive sorted queries of the item that owns it (wg_off); the grid is the host's upper
// bound ceil(cap / 64) + B, and the workgroups past the device's number leave at once.
template <int K, int PW>
__global__ __launch_bounds__(64 * PW) void knn_ragged_kernel(int B, int nk, int ntiles, int kout, RaggedWs ws,
                                                             int64_t* __restrict__ knn) {
  const int g = blockIdx.x;
  if (g >= ws.wg_off[B]) return;
  const int item = rk_find(ws.wg_off, B, g);
  const int pos = ws.lo[item] + (g - ws.wg_off[item]) * 64 + (threadIdx.x & 63);
  const bool live = pos < ws.lo[item + 1];
  knn_pruned_search<K, PW>(ws.qbuf, live, live ? ws.qorder[pos] : 0, ws.box + (int64_t)item * ntiles * 8,
                           ws.skey + (int64_t)item * nk * 3, ws.sidx + (int64_t)item * nk, ws.nvalid[item], ntiles, kout,
                           knn);
}

bool ragged_sizes_ok(int B, int64_t cap, int64_t nk, int k) {
  return k >= 1 && k <= 8 && B >= 1 && B <= MVK_KNN_RAGGED_MAX_ITEMS && cap >= 0 && nk >= 0 &&
         cap + (int64_t)B * nk < ((int64_t)1 << 30);
}

}  // namespace

extern "C" int64_t mvk_knn_ragged_workspace(int B, int64_t cap, int64_t nk, int k) {
  if (!ragged_sizes_ok(B, cap, nk, k)) return -1;
  return ragged_layout(B, cap, nk, true, nullptr, nullptr) + 256;
}

extern "C" int mvk_knn_f64_ragged(const float* points, int64_t N, const int64_t* rows, int64_t cap, const int64_t* q_off,
                                  int B, const double* keys, const uint8_t* key_valid, int64_t nk, int k, int64_t* knn,
                                  float* queries_out, void* workspace, int64_t workspace_bytes, void* stream) {
  MVK_REQUIRE(k >= 1 && k <= 8, "knn_ragged: k=%d unsupported (1..8)", k);
  MVK_REQUIRE(B >= 0 && cap >= 0 && nk >= 0 && N >= 0, "knn_ragged: bad sizes");
  if (B == 0 || cap == 0) return 0;
  MVK_REQUIRE(ragged_sizes_ok(B, cap, nk, k), "knn_ragged: B=%d (1..%d), cap + B * nk = %lld (< 2^30) refused", B,
              MVK_KNN_RAGGED_MAX_ITEMS, (long long)(cap + (int64_t)B * nk));
  MVK_REQUIRE(points && rows && q_off && knn && (keys || nk == 0), "knn_ragged: null pointer");
  MVK_REQUIRE(workspace && workspace_bytes >= mvk_knn_ragged_workspace(B, cap, nk, k), "knn_ragged: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  RaggedWs ws;
  char* base = (char*)(((uintptr_t)workspace + 255) / 256 * 256);
  ragged_layout(B, cap, nk, true, base, &ws);
  if (queries_out) ws.qbuf = queries_out;
  const int ntiles = (int)cdiv64(nk, PT);
  MVK_CHECK_HIP(hipMemsetAsync(ws.cnt, 0, (size_t)B * 2 * PNC * 4, st));
  hipLaunchKernelGGL(rk_plan_kernel, dim3(1), dim3(1024), 0, st, q_off, B, (int)cap, ws);
  const unsigned eb = (unsigned)cdiv64(cap + (int64_t)B * nk, 256);
  hipLaunchKernelGGL(rk_count_kernel, dim3(eb), dim3(256), 0, st, points, N, rows, (int)cap, B, keys, key_valid, (int)nk,
                     k, knn, ws);
  hipLaunchKernelGGL(rk_scan_kernel, dim3(2 * B), dim3(1024), 0, st, ws);
  hipLaunchKernelGGL(rk_scatter_kernel, dim3(eb), dim3(256), 0, st, (int)cap, B, keys, (int)nk, ws);
  if (ntiles > 0)
    hipLaunchKernelGGL(rk_box_kernel, dim3((unsigned)ntiles, (unsigned)B), dim3(64), 0, st, (int)nk, ntiles, ws);
  const dim3 grid((unsigned)(cdiv64(cap, 64) + B));
  if (k <= 3)
    hipLaunchKernelGGL((knn_ragged_kernel<3, 8>), grid, dim3(64 * 8), 0, st, B, (int)nk, ntiles, k, ws, knn);
  else
    hipLaunchKernelGGL((knn_ragged_kernel<8, 4>), grid, dim3(64 * 4), 0, st, B, (int)nk, ntiles, k, ws, knn);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

// =============================================================================================
// the sphere path
// =============================================================================================
namespace {

constexpr int SP_T = MVK_SPHERE_TILE;
constexpr int SP_WAVES = SP_T / 64;
constexpr int64_t MAX_GRID = ((int64_t)1 << 31) - 1;
static_assert(SP_T == COMPACT_T, "the member kernels scan their tile counts with compact.h");

// the smaller (value, index) pair, the lower index among equal values
__device__ __forceinline__ void take_lower(double& v, int64_t& i, double ov, int64_t oi) {
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// arg-min over the workgroup's SP_T threads; the result reaches every thread. s_v / s_i: SP_WAVES entries of LDS.
__device__ __forceinline__ void wg_argmin(double& v, int64_t& i, double* s_v, int64_t* s_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int64_t oi = (int64_t)__shfl_xor((long long)i, o);
    take_lower(v, i, ov, oi);
  }
  __syncthreads();                                   // the previous reduction's readers are done
  if ((threadIdx.x & 63) == 0) {
    s_v[threadIdx.x >> 6] = v;
    s_i[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = s_v[0];
  i = s_i[0];
  for (int w = 1; w < SP_WAVES; ++w) take_lower(v, i, s_v[w], s_i[w]);
}

__device__ __forceinline__ int64_t wg_sum(int64_t n, int64_t* s_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += (int64_t)__shfl_xor((long long)n, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_i[threadIdx.x >> 6] = n;
  __syncthreads();
  n = 0;
  for (int w = 0; w < SP_WAVES; ++w) n += s_i[w];
  return n;
}

__device__ __forceinline__ Ball ball_at(const float* __restrict__ c, double r2) {
  return Ball{(double)c[0], (double)c[1], (double)c[2], r2};
}

// potentials / min_potentials / argmin_potentials are read again after they were written (by the same thread, or behind a
// barrier): no __restrict__ on them.
__global__ __launch_bounds__(SP_T) void sphere_pick_k(const float* __restrict__ pot_points, int64_t PP, double* potentials,
                                                      const int64_t* __restrict__ pots, double* min_potentials,
                                                      int64_t* argmin_potentials, const float* __restrict__ points,
                                                      const int64_t* __restrict__ scenes, int S, Totals tot, double r2,
                                                      int64_t batch_limit, int B_max, int64_t* __restrict__ cloud_ind,
                                                      int64_t* __restrict__ point_ind, float* __restrict__ centers,
                                                      int32_t* __restrict__ lengths, int32_t* __restrict__ num_spheres) {
  __shared__ double s_v[SP_WAVES];
  __shared__ int64_t s_i[SP_WAVES];
  const int tid = threadIdx.x;
  int64_t batch_n = 0;
  int slot = 0;
  while (slot < B_max) {
    double bv = INFINITY;
    int64_t bi = INT64_MAX;
    for (int64_t s = tid; s < S; s += SP_T) take_lower(bv, bi, min_potentials[s], s);
    wg_argmin(bv, bi, s_v, s_i);
    const int64_t cloud = bi;
    if (cloud < 0 || cloud >= S) break;
    const Scene sc = load_scene(scenes, S, tot, cloud);
    const int64_t pot_off = pots[cloud * 2], num_pot = pots[cloud * 2 + 1], pt = argmin_potentials[cloud];
    if (!sc.ok || pot_off < 0 || num_pot < 1 || pot_off > PP || num_pot > PP - pot_off || pt < 0 || pt >= num_pot) break;
    const float* __restrict__ c = pot_points + (pot_off + pt) * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    const Ball b{(double)cx, (double)cy, (double)cz, r2};

    bv = INFINITY, bi = INT64_MAX;
    for (int64_t i = tid; i < num_pot; i += SP_T) {
      const double rd = ball_rdist(pot_points, pot_off + i, b);
      double p = potentials[pot_off + i];
      if (rd <= r2) {
        p += tukey_weight(rd, r2);
        potentials[pot_off + i] = p;
      }
      take_lower(bv, bi, p, i);
    }
    wg_argmin(bv, bi, s_v, s_i);

    int64_t n = 0;
    for (int64_t i = tid; i < sc.num_points; i += SP_T) n += ball_rdist(points, sc.point_off + i, b) <= r2 ? 1 : 0;
    n = wg_sum(n, s_i);

    if (tid == 0) {
      min_potentials[cloud] = bv;
      argmin_potentials[cloud] = bi;
      cloud_ind[slot] = cloud;
      point_ind[slot] = pt;
      centers[slot * 3] = cx, centers[slot * 3 + 1] = cy, centers[slot * 3 + 2] = cz;
      lengths[slot] = (int32_t)n;
    }
    __syncthreads();                                 // the next pick reads this cloud's new minimum
    batch_n += n;
    ++slot;
    if (batch_n > batch_limit) break;
  }
  for (int s = slot + tid; s < B_max; s += SP_T) {
    cloud_ind[s] = -1;
    point_ind[s] = -1;
    centers[s * 3] = centers[s * 3 + 1] = centers[s * 3 + 2] = 0.f;
    lengths[s] = 0;
  }
  if (tid == 0) *num_spheres = slot;
}

// the slot's scene, empty when it is larger than the grid was sized for
__device__ __forceinline__ Scene slot_scene(const int64_t* __restrict__ scenes, int S, const Totals& tot,
                                            const int64_t* __restrict__ cloud_ind, int b, int64_t max_points) {
  Scene sc = load_scene(scenes, S, tot, cloud_ind[b]);
  if (!sc.ok || sc.num_points > max_points) sc.num_points = 0;
  return sc;
}

// SCATTER false: the tile's member count -> block_counts. SCATTER true: block_counts hold the exclusive scan; the
// members' global indices go to the slot's row, cut at q_off[b + 1].
template <bool SCATTER>
__global__ __launch_bounds__(SP_T) void sphere_members_k(const float* __restrict__ points,
                                                         const int64_t* __restrict__ scenes, int S, Totals tot,
                                                         const int64_t* __restrict__ cloud_ind,
                                                         const float* __restrict__ centers, double r2, int bpi,
                                                         int64_t max_points, int32_t* __restrict__ block_counts,
                                                         const int64_t* __restrict__ q_off, int64_t* __restrict__ rows) {
  __shared__ int s_wc[SP_WAVES];
  const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
  const Scene sc = slot_scene(scenes, S, tot, cloud_ind, b, max_points);
  const int64_t n = sc.num_points;
  if ((int64_t)blk * SP_T >= n) return;
  const Ball ball = ball_at(centers + (int64_t)b * 3, r2);
  const int64_t i = (int64_t)blk * SP_T + threadIdx.x;
  const bool in = i < n && ball_rdist(points, sc.point_off + i, ball) <= r2;
  const unsigned long long m = __ballot(in);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_wc[wave] = __popcll(m);
  __syncthreads();
  if (!SCATTER) {
    if (threadIdx.x == 0) block_counts[(int64_t)b * bpi + blk] = compact_wave_offset(s_wc, SP_WAVES);
  } else if (in) {
    const int64_t at = q_off[b] + block_counts[(int64_t)b * bpi + blk] + compact_wave_offset(s_wc, wave) + compact_lane_rank(m);
    if (at < q_off[b + 1]) rows[at] = sc.point_off + i;
  }
}

// one workgroup: per slot the exclusive scan of its tile counts, and the slots' running sum -> q_off, cut to cap
__global__ __launch_bounds__(SP_T) void sphere_scan_k(const int64_t* __restrict__ scenes, int S, Totals tot,
                                                      const int64_t* __restrict__ cloud_ind, int B_max, int bpi,
                                                      int64_t max_points, int64_t cap, int32_t* __restrict__ block_counts,
                                                      int64_t* __restrict__ q_off, int32_t* __restrict__ status) {
  __shared__ int s_carry, s_ws[SP_WAVES];
  int64_t run = 0;
  for (int b = 0; b < B_max; ++b) {
    const Scene sc = slot_scene(scenes, S, tot, cloud_ind, b, max_points);
    const int members = compact_scan_counts(block_counts + (int64_t)b * bpi, (int)((sc.num_points + SP_T - 1) / SP_T), &s_carry, s_ws);
    if (threadIdx.x == 0) q_off[b] = run < cap ? run : cap;
    run += members;
    __syncthreads();                                 // s_carry is set again by the next slot's scan
  }
  if (threadIdx.x == 0) {
    q_off[B_max] = run < cap ? run : cap;
    if (run > cap) status[0] = 1;
  }
}

// LDS: alive [Wmax] words | count [max_frames] int32 (dynamic), the pick (static)
__global__ __launch_bounds__(SF_T) void sphere_select_frames_k(const uint32_t* __restrict__ bits,
                                                               const int64_t* __restrict__ base_point_ind,
                                                               const int64_t* __restrict__ scenes, int S, Totals tot,
                                                               const int64_t* __restrict__ cloud_ind,
                                                               const int64_t* __restrict__ mask_rows, int64_t cap,
                                                               const int64_t* __restrict__ mask_off, int nv, int max_base,
                                                               int max_frames, int Wmax, int32_t* __restrict__ sel) {
  extern __shared__ uint32_t s_mem[];
  __shared__ int s_pick;
  const int b = blockIdx.x;
  const Scene sc = load_scene(scenes, S, tot, cloud_ind[b]);
  if (!sc.ok || sc.num_base > max_base || sc.num_frames > max_frames || sc.num_frames < 1) {   // an empty slot: frame 0
    for (int r = threadIdx.x; r < nv; r += SF_T) sel[(int64_t)b * nv + r] = 0;
    return;
  }
  int64_t j0 = mask_off[b], j1 = mask_off[b + 1];
  if (j0 < 0 || j0 > cap || j1 < j0) j0 = j1 = 0;    // a row that leaves the buffer is cut to it
  else if (j1 > cap) j1 = cap;
  const int nb = (int)sc.num_base;
  select_frames_wg(bits + sc.bits_off, nb, (int)sc.num_frames, (nb + 31) >> 5, base_point_ind + sc.base_off, sc.point_off,
                   mask_rows + j0, j1 - j0, nv, sel + (int64_t)b * nv, s_mem, (int*)(s_mem + Wmax), &s_pick);
}

// the last b in [0, n] with v[b] <= x, -1 when there is none (n + 1 entries; any content stays in bounds)
__device__ __forceinline__ int find_slot(const int64_t* __restrict__ v, int n, int64_t x) {
  int a = 0, b = n + 1;
  while (a < b) {
    const int m = (a + b) >> 1;
    if (v[m] <= x) a = m + 1; else b = m;
  }
  return a - 1;
}

__global__ __launch_bounds__(256) void sphere_batch_rows_k(
    const float* __restrict__ points, const float* __restrict__ colors, const int64_t* __restrict__ labels,
    const int64_t* __restrict__ scenes, int S, Totals tot, const int64_t* __restrict__ cloud_ind,
    const float* __restrict__ centers, const int64_t* __restrict__ rows, int64_t cap, const int64_t* __restrict__ q_off,
    int B_max, const float* __restrict__ R, const float* __restrict__ scale, const float* __restrict__ noise,
    const float* __restrict__ keep_color, const int64_t* __restrict__ knn, int k, int64_t npix,
    float* __restrict__ aug_points, float* __restrict__ world, float* __restrict__ feat_aggre_points,
    float* __restrict__ colors_out, int64_t* __restrict__ labels_out, int64_t* __restrict__ knn_stacked,
    int64_t* __restrict__ input_inds) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  float aug[3] = {0.f, 0.f, 0.f}, wo[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f}, col[3] = {0.f, 0.f, 0.f};
  int64_t lab = 0, ind = -1;
  const int b = find_slot(q_off, B_max, i);
  bool ok = b >= 0 && b < B_max && i < q_off[b + 1];
  if (ok) {
    const Scene sc = load_scene(scenes, S, tot, cloud_ind[b]);
    const int64_t r = rows[i];
    ok = sc.ok && r >= sc.point_off && r < sc.point_off + sc.num_points;
    if (ok) {
      const float* __restrict__ c = centers + (int64_t)b * 3;
      const float* __restrict__ m = R + (int64_t)b * 9;
      const float* __restrict__ sc3 = scale + (int64_t)b * 3;
      const float keep = keep_color[b];
      float x[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        p[a] = points[r * 3 + a];
        x[a] = (float)((double)p[a] - (double)c[a]);
        col[a] = colors[r * 3 + a] * keep;
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        float v = ((x[0] * m[j] + x[1] * m[3 + j]) + x[2] * m[6 + j]) * sc3[j];
        if (noise) v = v + noise[i * 3 + j];
        aug[j] = v;
        wo[j] = (float)((double)v + (double)c[j]);
      }
      lab = labels[r];
      ind = r - sc.point_off;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    aug_points[i * 3 + a] = aug[a];
    world[i * 3 + a] = wo[a];
    feat_aggre_points[i * 3 + a] = p[a];
    colors_out[i * 3 + a] = col[a];
  }
  labels_out[i] = lab;
  input_inds[i] = ind;
  for (int c = 0; c < k; ++c) {
    const int64_t j = knn[i * k + c];
    knn_stacked[i * k + c] = ok && j >= 0 && j < npix ? j + (int64_t)b * npix : -1;
  }
}

}  // namespace

extern "C" int mvk_sphere_pick(const float* pot_points, int64_t PP, double* potentials, const int64_t* pots,
                               double* min_potentials, int64_t* argmin_potentials, const float* points, int64_t P,
                               const int64_t* scenes, int S, int64_t NB, int64_t F, int64_t NW, double in_radius,
                               int64_t batch_limit, int B_max, int64_t* cloud_ind, int64_t* point_ind, float* centers,
                               int32_t* lengths, int32_t* num_spheres, void* stream) {
  MVK_REQUIRE(totals_ok(P, NB, F, NW, S) && PP >= 0 && PP < MAX_SIZE && B_max >= 0 && B_max <= MVK_SPHERE_MAX_SLOTS,
              "sphere_pick: bad sizes or sizes of 2^31 or more (P=%lld NB=%lld F=%lld NW=%lld S=%d PP=%lld B_max=%d, <= %d "
              "slots)", (long long)P, (long long)NB, (long long)F, (long long)NW, S, (long long)PP, B_max,
              MVK_SPHERE_MAX_SLOTS);
  MVK_REQUIRE(in_radius > 0.0, "sphere_pick: in_radius must be positive");
  if (B_max == 0) return 0;
  MVK_REQUIRE(cloud_ind && point_ind && centers && lengths && num_spheres &&
                  (S == 0 || (scenes && pots && min_potentials && argmin_potentials)) &&
                  (PP == 0 || (pot_points && potentials)) && (points || P == 0),
              "sphere_pick: null operand");
  const Totals tot = {P, NB, F, NW};
  hipLaunchKernelGGL(sphere_pick_k, dim3(1), dim3(SP_T), 0, (hipStream_t)stream, pot_points, PP, potentials, pots,
                     min_potentials, argmin_potentials, points, scenes, S, tot, in_radius * in_radius, batch_limit, B_max,
                     cloud_ind, point_ind, centers, lengths, num_spheres);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_sphere_members(const float* points, int64_t P, const int64_t* scenes, int S, int64_t NB, int64_t F,
                                  int64_t NW, const int64_t* cloud_ind, const float* centers, int B_max, double radius,
                                  int64_t max_points, int64_t cap, int32_t* block_counts, int64_t* rows, int64_t* q_off,
                                  int32_t* status, void* stream) {
  MVK_REQUIRE(totals_ok(P, NB, F, NW, S) && B_max >= 0 && B_max <= MVK_SPHERE_MAX_SLOTS && max_points >= 0 &&
                  max_points < MAX_SIZE && cap >= 0 && cap < MAX_SIZE && radius >= 0.0,
              "sphere_members: bad sizes or sizes of 2^31 or more (P=%lld NB=%lld F=%lld NW=%lld S=%d B_max=%d "
              "max_points=%lld cap=%lld)", (long long)P, (long long)NB, (long long)F, (long long)NW, S, B_max,
              (long long)max_points, (long long)cap);
  const int64_t bpi = max_points > 0 ? cdiv64(max_points, SP_T) : 1;
  MVK_REQUIRE((int64_t)B_max * bpi <= MAX_GRID, "sphere_members: sizes of 2^31 or more (B_max=%d max_points=%lld)", B_max,
              (long long)max_points);
  if (B_max == 0) return 0;
  MVK_REQUIRE(scenes && cloud_ind && centers && block_counts && q_off && status && (points || P == 0) && (rows || cap == 0),
              "sphere_members: null operand");
  hipStream_t st = (hipStream_t)stream;
  const Totals tot = {P, NB, F, NW};
  const dim3 grid((unsigned)(B_max * bpi));
  const double r2 = radius * radius;
  hipLaunchKernelGGL(sphere_members_k<false>, grid, dim3(SP_T), 0, st, points, scenes, S, tot, cloud_ind, centers, r2,
                     (int)bpi, max_points, block_counts, (const int64_t*)q_off, rows);
  hipLaunchKernelGGL(sphere_scan_k, dim3(1), dim3(SP_T), 0, st, scenes, S, tot, cloud_ind, B_max, (int)bpi, max_points, cap,
                     block_counts, q_off, status);
  hipLaunchKernelGGL(sphere_members_k<true>, grid, dim3(SP_T), 0, st, points, scenes, S, tot, cloud_ind, centers, r2,
                     (int)bpi, max_points, block_counts, (const int64_t*)q_off, rows);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_sphere_select_frames(const int32_t* bits, int64_t NW, const int64_t* base_point_ind, int64_t NB,
                                        const int64_t* scenes, int S, int64_t P, int64_t F, const int64_t* cloud_ind,
                                        const int64_t* mask_rows, int64_t cap, const int64_t* mask_off, int B_max, int nv,
                                        int64_t max_base, int64_t max_frames, int32_t* sel, void* stream) {
  MVK_REQUIRE(totals_ok(P, NB, F, NW, S) && cap >= 0 && cap < MAX_SIZE && B_max >= 0 && B_max <= MVK_SPHERE_MAX_SLOTS &&
                  nv >= 0 && max_base >= 0 && max_frames >= 0 && (int64_t)B_max * nv < MAX_SIZE,
              "sphere_select_frames: bad sizes or sizes of 2^31 or more (P=%lld NB=%lld F=%lld NW=%lld S=%d cap=%lld "
              "B_max=%d nv=%d)", (long long)P, (long long)NB, (long long)F, (long long)NW, S, (long long)cap, B_max, nv);
  MVK_REQUIRE(max_base <= MVK_SCENE_MAX_BASE && max_frames <= MVK_SCENE_MAX_FRAMES,
              "sphere_select_frames: max_base=%lld base points (<= %d) or max_frames=%lld frames (<= %d) exceed the "
              "kernel's LDS; there is no fallback", (long long)max_base, MVK_SCENE_MAX_BASE, (long long)max_frames,
              MVK_SCENE_MAX_FRAMES);
  if (B_max == 0 || nv == 0) return 0;
  MVK_REQUIRE(sel && scenes && cloud_ind && mask_off && (bits || NW == 0) && (base_point_ind || NB == 0) &&
                  (mask_rows || cap == 0),
              "sphere_select_frames: null operand");
  const int Wmax = (int)cdiv64(max_base, 32);
  const int64_t lds = ((int64_t)Wmax + max_frames) * 4;
  if (lds > 64 * 1024)
    MVK_CHECK_HIP(hipFuncSetAttribute((const void*)sphere_select_frames_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const Totals tot = {P, NB, F, NW};
  hipLaunchKernelGGL(sphere_select_frames_k, dim3(B_max), dim3(SF_T), (size_t)lds, (hipStream_t)stream,
                     (const uint32_t*)bits, base_point_ind, scenes, S, tot, cloud_ind, mask_rows, cap, mask_off, nv,
                     (int)max_base, (int)max_frames, Wmax, sel);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_sphere_batch_rows(const float* points, const float* colors, const int64_t* labels, int64_t P,
                                     const int64_t* scenes, int S, int64_t NB, int64_t F, int64_t NW,
                                     const int64_t* cloud_ind, const float* centers, const int64_t* rows, int64_t cap,
                                     const int64_t* q_off, int B_max, const float* R, const float* scale,
                                     const float* noise, const float* keep_color, const int64_t* knn, int k, int64_t npix,
                                     float* aug_points, float* world, float* feat_aggre_points, float* colors_out,
                                     int64_t* labels_out, int64_t* knn_stacked, int64_t* input_inds, void* stream) {
  MVK_REQUIRE(totals_ok(P, NB, F, NW, S) && cap >= 0 && cap < MAX_SIZE / 8 && B_max >= 0 && B_max <= MVK_SPHERE_MAX_SLOTS &&
                  k >= 0 && k <= 8 && npix >= 0 && npix < MAX_SIZE,
              "sphere_batch_rows: bad sizes (P=%lld NB=%lld F=%lld NW=%lld S=%d cap=%lld B_max=%d k=%d npix=%lld)",
              (long long)P, (long long)NB, (long long)F, (long long)NW, S, (long long)cap, B_max, k, (long long)npix);
  if (cap == 0) return 0;
  MVK_REQUIRE(q_off && aug_points && world && feat_aggre_points && colors_out && labels_out && input_inds &&
                  (k == 0 || (knn && knn_stacked)) &&
                  (B_max == 0 || (scenes && cloud_ind && centers && rows && R && scale && keep_color)) &&
                  ((points && colors && labels) || P == 0),
              "sphere_batch_rows: null operand");
  const Totals tot = {P, NB, F, NW};
  hipLaunchKernelGGL(sphere_batch_rows_k, dim3((unsigned)cdiv64(cap, 256)), dim3(256), 0, (hipStream_t)stream, points,
                     colors, labels, scenes, S, tot, cloud_ind, centers, rows, cap, q_off, B_max, R, scale, noise,
                     keep_color, knn, k, npix, aug_points, world, feat_aggre_points, colors_out, labels_out, knn_stacked,
                     input_inds);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
