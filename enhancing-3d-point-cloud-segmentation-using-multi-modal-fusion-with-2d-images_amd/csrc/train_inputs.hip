// The training batches of the MVPNet baseline from scenes resident in HBM, B items of B scenes at a time
// (include/mvkpconv_train.h; reference: mvpnet/data/scannet_2d3d.py:323-416 with get_rgbd_data, :191-321, which is NumPy
// in DataLoader workers: ten tries at a crop, a resample, a greedy frame choice, three unprojections and a ball tree).
//   pick_count_k            cnt / lab of all T tries in one pass over the item's scene: ballots, LDS counters, one integer
//                           atomic per (try, counter) and workgroup
//   pick_members_k<false>   the chosen try (recomputed from the counts by every workgroup: T reads) and the members of
//                           its box per 1024-point tile
//   pick_scan_k             one workgroup per item: exclusive scan of the tile counts (compact.h), row_len, and the
//                           whole-scene box (min / max xy) of an item without a valid try
//   pick_members_k<true>    the members' global indices at tile offset + rank: ascending, np.nonzero's order
//   resample_k              one workgroup per item: a radix select (8 bits a pass) of the nb_pts-th smallest (key,
//                           position), then an ordered compaction in passes of 1024 positions with the rank among equal
//                           keys from a second scan; keys are recomputed, never stored
//   train_select_frames_k   select_frames.h's greedy coverage on the item's own bit rows
//   train_unproject_k       unproject.h's expression with the item's intrinsics, the box mask, the per-view flip and the
//                           rotation of the float32 copy
//   train_batch_rows_k      the rotated points [B,3,nb_pts] and the labels
// The k-NN between them is mvk_chunk_knn_many (csrc/scene_inputs.hip), unchanged.
// Integer arithmetic, or floats in the written order (-ffp-contract=off). The only atomics are integer counters summed
// in LDS first. A workgroup never straddles two items, so per-item values are read at wave-uniform addresses.
#include "common.h"
#include "compact.h"
#include "resident.h"
#include "select_frames.h"
#include "unproject.h"
#include "../../include/mvkpconv_scene.h"
#include "../../include/mvkpconv_train.h"

namespace {

constexpr int PK_T = MVK_TRAIN_PICK_TILE;          // points (threads) per pick workgroup
constexpr int PK_WAVES = PK_T / 64;
constexpr int RS_T = MVK_TRAIN_RESAMPLE_STRIDE;    // threads of the resample workgroup = positions per pass
constexpr int RS_WAVES = RS_T / 64;
constexpr int UP_T = 256;                          // threads of the unprojection kernel
constexpr int BR_T = 256;                          // threads of the row kernel
constexpr int MAX_T = MVK_TRAIN_MAX_TRIES;
constexpr int64_t MAX_GRID = ((int64_t)1 << 31) - 1;
constexpr int64_t IGNORE_LABEL = -100;
static_assert(PK_T == COMPACT_T, "the pick kernels scan their tile counts with compact.h");

struct Crop {
  float sx, sy, mx, my;
};

// the box of a try around point c of the scene, in float32 in the header's order
__device__ __forceinline__ void try_box(const float* __restrict__ points, const Scene& sc, int64_t c, const Crop& cr,
                                        float (&lo)[2], float (&hi)[2]) {
  const float cx = points[(sc.point_off + c) * 3], cy = points[(sc.point_off + c) * 3 + 1];
  lo[0] = (cx - 0.5f * cr.sx) - cr.mx;
  lo[1] = (cy - 0.5f * cr.sy) - cr.my;
  hi[0] = (cx + 0.5f * cr.sx) + cr.mx;
  hi[1] = (cy + 0.5f * cr.sy) + cr.my;
}

__device__ __forceinline__ bool inside(float x, float y, const float* lo, const float* hi) {
  return x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1];
}

// the first try with a point and enough labeled ones, or -1
__device__ __forceinline__ int decide(const int32_t* __restrict__ counts, int T, double thresh) {
  for (int t = 0; t < T; ++t) {
    const int cnt = counts[2 * t], lab = counts[2 * t + 1];
    if (cnt > 0 && (double)lab / (double)cnt >= thresh) return t;
  }
  return -1;
}

__global__ __launch_bounds__(PK_T) void pick_count_k(const float* __restrict__ points, const int64_t* __restrict__ labels,
                                                     const int64_t* __restrict__ scenes, int S, Totals tot,
                                                     const int64_t* __restrict__ scene_id,
                                                     const int64_t* __restrict__ centers, int T, int bpi,
                                                     int64_t max_points, Crop cr, int32_t* __restrict__ counts) {
  __shared__ float s_lo[MAX_T][2], s_hi[MAX_T][2];
  __shared__ int s_ok[MAX_T], s_cnt[MAX_T][2];
  const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
  const Scene sc = load_scene(scenes, S, tot, scene_id[b]);
  const int64_t n = sc.num_points <= max_points ? sc.num_points : 0;
  if ((int64_t)blk * PK_T >= n) return;
  if (threadIdx.x < T) {
    const int t = threadIdx.x;
    const int64_t c = centers[(int64_t)b * T + t];
    const bool ok = c >= 0 && c < n;
    float lo[2] = {0.f, 0.f}, hi[2] = {0.f, 0.f};
    if (ok) try_box(points, sc, c, cr, lo, hi);
    s_lo[t][0] = lo[0], s_lo[t][1] = lo[1], s_hi[t][0] = hi[0], s_hi[t][1] = hi[1];
    s_ok[t] = ok;
    s_cnt[t][0] = s_cnt[t][1] = 0;
  }
  __syncthreads();
  const int64_t i = (int64_t)blk * PK_T + threadIdx.x;
  const bool here = i < n;
  float x = 0.f, y = 0.f;
  bool labeled = false;
  if (here) {
    x = points[(sc.point_off + i) * 3];
    y = points[(sc.point_off + i) * 3 + 1];
    labeled = labels[sc.point_off + i] >= 0;
  }
  for (int t = 0; t < T; ++t) {
    const bool in = here && s_ok[t] && inside(x, y, s_lo[t], s_hi[t]);
    const unsigned long long m = __ballot(in), ml = __ballot(in && labeled);
    if ((threadIdx.x & 63) == 0) {
      if (m) atomicAdd(&s_cnt[t][0], __popcll(m));
      if (ml) atomicAdd(&s_cnt[t][1], __popcll(ml));
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * T) {
    const int v = s_cnt[threadIdx.x >> 1][threadIdx.x & 1];
    if (v) atomicAdd(&counts[(int64_t)b * T * 2 + threadIdx.x], v);
  }
}

// SCATTER false: the tile's member count -> block_counts, and chosen / the try's box by the item's first workgroup.
// SCATTER true: block_counts hold the exclusive scan; the members' global indices go to the row.
template <bool SCATTER>
__global__ __launch_bounds__(PK_T) void pick_members_k(const float* __restrict__ points,
                                                       const int64_t* __restrict__ scenes, int S, Totals tot,
                                                       const int64_t* __restrict__ scene_id,
                                                       const int64_t* __restrict__ centers, int T, int bpi,
                                                       int64_t max_points, Crop cr, double thresh,
                                                       const int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ block_counts, int32_t* __restrict__ chosen_out,
                                                       float* __restrict__ box_out, const int64_t* __restrict__ row_off,
                                                       const int64_t* __restrict__ row_len, int64_t* __restrict__ rows) {
  __shared__ int s_chosen, s_wc[PK_WAVES];
  __shared__ float s_lo[2], s_hi[2];
  const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
  const Scene sc = load_scene(scenes, S, tot, scene_id[b]);
  const int64_t n = sc.num_points <= max_points ? sc.num_points : 0;
  if (blk > 0 && (int64_t)blk * PK_T >= n) return;
  if (threadIdx.x == 0) {
    const int chosen = decide(counts + (int64_t)b * T * 2, T, thresh);
    float lo[2] = {0.f, 0.f}, hi[2] = {0.f, 0.f};
    if (chosen >= 0) try_box(points, sc, centers[(int64_t)b * T + chosen], cr, lo, hi);   // cnt > 0: the centre is a point
    s_chosen = chosen;
    s_lo[0] = lo[0], s_lo[1] = lo[1], s_hi[0] = hi[0], s_hi[1] = hi[1];
    if (!SCATTER && blk == 0) {
      chosen_out[b] = chosen;
      if (chosen >= 0) box_out[b * 4] = lo[0], box_out[b * 4 + 1] = lo[1], box_out[b * 4 + 2] = hi[0], box_out[b * 4 + 3] = hi[1];
    }
  }
  __syncthreads();
  const int64_t i = (int64_t)blk * PK_T + threadIdx.x;
  bool in = i < n;
  if (in && s_chosen >= 0) in = inside(points[(sc.point_off + i) * 3], points[(sc.point_off + i) * 3 + 1], s_lo, s_hi);
  const unsigned long long m = __ballot(in);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_wc[wave] = __popcll(m);
  __syncthreads();
  if (!SCATTER) {
    if (threadIdx.x == 0) block_counts[(int64_t)b * bpi + blk] = compact_wave_offset(s_wc, PK_WAVES);
  } else if (in) {
    const int64_t at = (int64_t)block_counts[(int64_t)b * bpi + blk] + compact_wave_offset(s_wc, wave) + compact_lane_rank(m);
    if (at < row_len[b]) rows[row_off[b] + at] = sc.point_off + i;      // row_len is cut to the row's capacity
  }
}

__global__ __launch_bounds__(PK_T) void pick_scan_k(const float* __restrict__ points, const int64_t* __restrict__ scenes,
                                                    int S, Totals tot, const int64_t* __restrict__ scene_id, int T, int bpi,
                                                    int64_t max_points, Crop cr, double thresh,
                                                    const int32_t* __restrict__ counts, int32_t* __restrict__ block_counts,
                                                    const int64_t* __restrict__ row_off, int64_t total,
                                                    float* __restrict__ box_out, int64_t* __restrict__ row_len) {
  __shared__ int s_carry, s_ws[PK_WAVES];
  __shared__ float s_min[PK_WAVES][2], s_max[PK_WAVES][2];
  const int b = blockIdx.x;
  const Scene sc = load_scene(scenes, S, tot, scene_id[b]);
  const int64_t n = sc.num_points <= max_points ? sc.num_points : 0;
  const int members = compact_scan_counts(block_counts + (int64_t)b * bpi, (int)((n + PK_T - 1) / PK_T), &s_carry, s_ws);
  if (threadIdx.x == 0) {
    const int64_t j0 = row_off[b];
    int64_t len = members;
    if (j0 < 0 || j0 > total) len = 0;                                 // a row that leaves the buffer is cut to it
    else if (len > total - j0) len = total - j0;
    row_len[b] = len;
  }
  if (decide(counts + (int64_t)b * T * 2, T, thresh) >= 0) return;     // wave-uniform: the box is the try's
  // no valid try: the whole scene, its min / max xy with the margin (float32; min and max are exact in any order)
  float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  for (int64_t i = threadIdx.x; i < n; i += PK_T) {
    const float x = points[(sc.point_off + i) * 3], y = points[(sc.point_off + i) * 3 + 1];
    lo[0] = fminf(lo[0], x), lo[1] = fminf(lo[1], y), hi[0] = fmaxf(hi[0], x), hi[1] = fmaxf(hi[1], y);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], o));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o));
    }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_min[wave][0] = lo[0], s_min[wave][1] = lo[1], s_max[wave][0] = hi[0], s_max[wave][1] = hi[1];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < PK_WAVES; ++k)
      for (int a = 0; a < 2; ++a) lo[a] = fminf(lo[a], s_min[k][a]), hi[a] = fmaxf(hi[a], s_max[k][a]);
    float* __restrict__ box = box_out + (int64_t)b * 4;
    if (n > 0) box[0] = lo[0] - cr.mx, box[1] = lo[1] - cr.my, box[2] = hi[0] + cr.mx, box[3] = hi[1] + cr.my;
    else box[0] = box[1] = box[2] = box[3] = 0.f;
  }
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t draw32(uint32_t seed_lo, uint32_t seed_hi, uint32_t i) {
  return mix32(seed_lo ^ mix32(seed_hi + i * 0x9e3779b9u));
}

__global__ __launch_bounds__(RS_T) void resample_k(const int64_t* __restrict__ rows, int64_t total,
                                                   const int64_t* __restrict__ row_off, const int64_t* __restrict__ row_len,
                                                   const int64_t* __restrict__ seeds, int64_t nb_pts, int key_bits,
                                                   int64_t* __restrict__ sample_rows, int32_t* __restrict__ sample_pos) {
  __shared__ unsigned s_hist[256], s_prefix, s_remaining;
  __shared__ int s_we[RS_WAVES], s_wt[RS_WAVES];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t j0 = row_off[b], nc = row_len[b];
  if (j0 < 0 || j0 > total || nc < 0) nc = 0;                          // a row that leaves the buffer is cut to it
  else if (nc > total - j0) nc = total - j0;
  const int64_t* __restrict__ row = rows + (nc > 0 ? j0 : 0);
  const uint32_t seed_lo = (uint32_t)(uint64_t)seeds[b], seed_hi = (uint32_t)((uint64_t)seeds[b] >> 32);
  int64_t* __restrict__ out_rows = sample_rows + (int64_t)b * nb_pts;
  int32_t* __restrict__ out_pos = sample_pos + (int64_t)b * nb_pts;

  if (nc < nb_pts) {                                                   // the row, then the pads (none of an empty row)
    for (int64_t j = threadIdx.x; j < nb_pts; j += RS_T) {
      int64_t pos = -1;
      if (nc > 0) pos = j < nc ? j : (int64_t)(((uint64_t)draw32(seed_lo, seed_hi, (uint32_t)j) * (uint64_t)nc) >> 32);
      out_pos[j] = (int32_t)pos;
      out_rows[j] = pos >= 0 ? row[pos] : -1;
    }
    return;
  }
  if (nb_pts == 0) return;

  // radix select: K = the key of the nb_pts-th entry in (key, position) order, r = how many of its equals are taken
  const int drop = 32 - key_bits;
  if (threadIdx.x == 0) s_prefix = 0u, s_remaining = (unsigned)nb_pts;
  __syncthreads();
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (shift >= key_bits) continue;                                   // these digits of every key are zero
    if (threadIdx.x < 256) s_hist[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned prefix = s_prefix;
    for (int64_t i = threadIdx.x; i < nc; i += RS_T) {
      const uint32_t k = draw32(seed_lo, seed_hi, (uint32_t)i) >> drop;
      if (shift == 24 || (k >> (shift + 8)) == prefix) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned left = s_remaining, d = 0;
      while (d < 255u && s_hist[d] < left) left -= s_hist[d++];
      s_prefix = (prefix << 8) | d;
      s_remaining = left;
    }
    __syncthreads();
  }
  const uint32_t K = s_prefix;
  const int r = (int)s_remaining;

  // ordered compaction: every key below K, and the first r positions whose key is K
  int64_t tie_base = 0, out_base = 0;
  for (int64_t base = 0; base < nc && out_base < nb_pts; base += RS_T) {
    const int64_t i = base + threadIdx.x;
    const uint32_t k = draw32(seed_lo, seed_hi, (uint32_t)i) >> drop;
    const bool lt = i < nc && k < K, eq = i < nc && k == K;
    const unsigned long long me = __ballot(eq);
    if (lane == 0) s_we[wave] = __popcll(me);
    __syncthreads();
    const int64_t tie_rank = tie_base + compact_wave_offset(s_we, wave) + compact_lane_rank(me);
    tie_base += compact_wave_offset(s_we, RS_WAVES);
    const bool take = lt || (eq && tie_rank < r);
    const unsigned long long mt = __ballot(take);
    if (lane == 0) s_wt[wave] = __popcll(mt);
    __syncthreads();
    if (take) {
      const int64_t at = out_base + compact_wave_offset(s_wt, wave) + compact_lane_rank(mt);
      if (at < nb_pts) {                                               // exactly nb_pts are taken; never write past them
        out_pos[at] = (int32_t)i;
        out_rows[at] = row[i];
      }
    }
    out_base += compact_wave_offset(s_wt, RS_WAVES);
  }
}

// LDS: alive [Wmax] words | count [max_frames] int32 (dynamic), the pick (static)
__global__ __launch_bounds__(SF_T) void train_select_frames_k(const uint32_t* __restrict__ bits,
                                                              const int64_t* __restrict__ base_point_ind,
                                                              const int64_t* __restrict__ scenes, int S, Totals tot,
                                                              const int64_t* __restrict__ scene_id,
                                                              const int64_t* __restrict__ rows, int64_t total,
                                                              const int64_t* __restrict__ row_off,
                                                              const int64_t* __restrict__ row_len, int nv, int max_base,
                                                              int max_frames, int Wmax, int32_t* __restrict__ sel) {
  extern __shared__ uint32_t s_mem[];
  __shared__ int s_pick;
  const int b = blockIdx.x;
  const Scene sc = load_scene(scenes, S, tot, scene_id[b]);
  if (!sc.ok || sc.num_base > max_base || sc.num_frames > max_frames || sc.num_frames < 1) {   // an empty item: frame 0
    for (int r = threadIdx.x; r < nv; r += SF_T) sel[(int64_t)b * nv + r] = 0;
    return;
  }
  int64_t j0 = row_off[b], n = row_len[b];
  if (j0 < 0 || j0 > total || n < 0) n = 0;
  else if (n > total - j0) n = total - j0;
  const int nb = (int)sc.num_base;
  select_frames_wg(bits + sc.bits_off, nb, (int)sc.num_frames, (nb + 31) >> 5, base_point_ind + sc.base_off, sc.point_off,
                   rows + (n > 0 ? j0 : 0), n, nv, sel + (int64_t)b * nv, s_mem, (int*)(s_mem + Wmax), &s_pick);
}

// m[r][0]*x + m[r][1]*y + m[r][2]*z in float64, left to right, rounded to float32
__device__ __forceinline__ float rotated(const double* __restrict__ m, int r, float x, float y, float z) {
  return (float)((m[r * 3] * (double)x + m[r * 3 + 1] * (double)y) + m[r * 3 + 2] * (double)z);
}

__global__ __launch_bounds__(UP_T) void train_unproject_k(const int32_t* __restrict__ sel,
                                                          const int64_t* __restrict__ scene_id, int nv,
                                                          const int64_t* __restrict__ scenes, int S, Totals tot,
                                                          const uint16_t* __restrict__ depth,
                                                          const float* __restrict__ images_in,
                                                          const float* __restrict__ poses,
                                                          const double* __restrict__ cam_inv, int h, int w,
                                                          int blocks_per_item, const float* __restrict__ box,
                                                          const uint8_t* __restrict__ flips, const double* __restrict__ rot,
                                                          double* __restrict__ keys, float* __restrict__ image_xyz,
                                                          uint8_t* __restrict__ image_mask, float* __restrict__ images_out,
                                                          int32_t* __restrict__ num_valid) {
  __shared__ int s_n;
  const int b = blockIdx.x / blocks_per_item;                          // one item per workgroup
  const int64_t hw = (int64_t)h * w, Pix = (int64_t)nv * hw;
  const int64_t p = (int64_t)(blockIdx.x - b * blocks_per_item) * UP_T + threadIdx.x;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int64_t sid = scene_id[b];
  const Scene sc = load_scene(scenes, S, tot, sid);                    // wave-uniform
  bool valid = false;
  if (p < Pix) {
    const int view = (int)(p / hw);
    const int64_t pix = p - view * hw;
    const int f = sel[(int64_t)b * nv + view];
    const int64_t out = (int64_t)b * Pix + p;
    float rgb[3] = {0.f, 0.f, 0.f}, xf[3] = {0.f, 0.f, 0.f};
    double c[3] = {0.0, 0.0, 0.0}, x[3] = {0.0, 0.0, 0.0};
    if (sc.ok && f >= 0 && f < sc.num_frames) {
      const int64_t frame = sc.frame_off + f;
      const int64_t row = pix / w, col = pix - row * w;
      const int64_t scol = flips && flips[(int64_t)b * nv + view] ? w - 1 - col : col;
      const int64_t src = frame * hw + row * w + scol;
      Cam cam;
#pragma unroll
      for (int i = 0; i < 9; ++i) cam.kinv[i] = cam_inv[sid * 9 + i];
      unproject_pixel(cam, poses + frame * 16, (double)scol, (double)row, depth[src], c, x);
      const float* __restrict__ bx = box + (int64_t)b * 4;             // (lo.x, lo.y, hi.x, hi.y)
      valid = c[2] > 0.0 && x[0] > (double)bx[0] - 0.1 && x[0] < (double)bx[2] + 0.1 && x[1] > (double)bx[1] - 0.1 &&
              x[1] < (double)bx[3] + 0.1;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) rgb[ch] = images_in[src * 3 + ch];
#pragma unroll
      for (int r = 0; r < 3; ++r) xf[r] = (float)x[r];
      if (rot) {
        const double* __restrict__ m = rot + (int64_t)b * 9;
        const float x0 = xf[0], x1 = xf[1], x2 = xf[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) xf[r] = rotated(m, r, x0, x1, x2);
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      keys[out * 3 + r] = x[r];
      image_xyz[out * 3 + r] = xf[r];
      images_out[(((int64_t)b * nv + view) * 3 + r) * hw + pix] = rgb[r];
    }
    image_mask[out] = valid ? 1 : 0;
  }
  const unsigned long long m = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_n, __popcll(m));
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(&num_valid[b], s_n);
}

__global__ __launch_bounds__(BR_T) void train_batch_rows_k(const float* __restrict__ queries,
                                                           const int64_t* __restrict__ labels, int64_t P,
                                                           const int64_t* __restrict__ sample_rows,
                                                           const double* __restrict__ rot, int blocks_per_item,
                                                           int64_t nb_pts, float* __restrict__ points_out,
                                                           int64_t* __restrict__ seg_label) {
  const int b = blockIdx.x / blocks_per_item;                          // one item per workgroup
  const int64_t j = (int64_t)(blockIdx.x - b * blocks_per_item) * BR_T + threadIdx.x;
  if (j >= nb_pts) return;
  const int64_t q = (int64_t)b * nb_pts + j;
  const float x = queries[q * 3], y = queries[q * 3 + 1], z = queries[q * 3 + 2];
  float o[3] = {x, y, z};
  if (rot) {
    const double* __restrict__ m = rot + (int64_t)b * 9;               // wave-uniform
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = rotated(m, r, x, y, z);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) points_out[((int64_t)b * 3 + r) * nb_pts + j] = o[r];
  const int64_t i = sample_rows[q];
  seg_label[q] = i >= 0 && i < P ? labels[i] : IGNORE_LABEL;
}

}  // namespace

extern "C" int mvk_train_chunk_pick(const float* points, const int64_t* labels, int64_t P, const int64_t* scenes, int S,
                                    int64_t NB, int64_t F, int64_t NW, const int64_t* scene_id, const int64_t* centers,
                                    int B, int T, float size_x, float size_y, float margin_x, float margin_y,
                                    double chunk_thresh, int64_t max_points, const int64_t* row_off, int64_t total,
                                    int32_t* block_counts, int32_t* counts, int32_t* chosen, float* box, int64_t* rows,
                                    int64_t* row_len, void* stream) {
  MVK_REQUIRE(totals_ok(P, NB, F, NW, S) && B >= 0 && T >= 0 && max_points >= 0 && total >= 0 && max_points < MAX_SIZE &&
                  total < MAX_SIZE,
              "train_chunk_pick: bad sizes or sizes of 2^31 or more (P=%lld NB=%lld F=%lld NW=%lld S=%d B=%d T=%d "
              "max_points=%lld total=%lld)", (long long)P, (long long)NB, (long long)F, (long long)NW, S, B, T,
              (long long)max_points, (long long)total);
  MVK_REQUIRE(T <= MVK_TRAIN_MAX_TRIES, "train_chunk_pick: T=%d tries (<= %d: their boxes and counters live in LDS)", T,
              MVK_TRAIN_MAX_TRIES);
  const int64_t bpi = max_points > 0 ? cdiv64(max_points, PK_T) : 1;
  MVK_REQUIRE((int64_t)B * bpi <= MAX_GRID && (int64_t)B * (T > 2 ? T : 2) * 2 < MAX_SIZE,
              "train_chunk_pick: sizes of 2^31 or more (B=%d T=%d max_points=%lld)", B, T, (long long)max_points);
  if (B == 0) return 0;
  MVK_REQUIRE(scenes && scene_id && row_off && block_counts && chosen && box && row_len && (centers || T == 0) &&
                  (counts || T == 0) && (points || P == 0) && (labels || P == 0) && (rows || total == 0),
              "train_chunk_pick: null operand");
  hipStream_t st = (hipStream_t)stream;
  const Totals tot = {P, NB, F, NW};
  const Crop cr = {size_x, size_y, margin_x, margin_y};
  const dim3 grid((unsigned)(B * bpi));
  if (T > 0) {
    MVK_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * T * 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(pick_count_k, grid, dim3(PK_T), 0, st, points, labels, scenes, S, tot, scene_id, centers, T, (int)bpi,
                       max_points, cr, counts);
    MVK_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(pick_members_k<false>, grid, dim3(PK_T), 0, st, points, scenes, S, tot, scene_id, centers, T, (int)bpi,
                     max_points, cr, chunk_thresh, (const int32_t*)counts, block_counts, chosen, box, row_off,
                     (const int64_t*)row_len, rows);
  MVK_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(pick_scan_k, dim3(B), dim3(PK_T), 0, st, points, scenes, S, tot, scene_id, T, (int)bpi, max_points, cr,
                     chunk_thresh, (const int32_t*)counts, block_counts, row_off, total, box, row_len);
  MVK_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(pick_members_k<true>, grid, dim3(PK_T), 0, st, points, scenes, S, tot, scene_id, centers, T, (int)bpi,
                     max_points, cr, chunk_thresh, (const int32_t*)counts, block_counts, chosen, box, row_off,
                     (const int64_t*)row_len, rows);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_train_chunk_resample(const int64_t* rows, int64_t total, const int64_t* row_off, const int64_t* row_len,
                                        const int64_t* seeds, int B, int64_t nb_pts, int key_bits, int64_t* sample_rows,
                                        int32_t* sample_pos, void* stream) {
  MVK_REQUIRE(total >= 0 && B >= 0 && nb_pts >= 0 && total < MAX_SIZE && nb_pts < MAX_SIZE &&
                  (nb_pts == 0 || B < MAX_SIZE / nb_pts),
              "train_chunk_resample: bad sizes or sizes of 2^31 or more (total=%lld B=%d nb_pts=%lld)", (long long)total, B,
              (long long)nb_pts);
  MVK_REQUIRE(key_bits >= 1 && key_bits <= 32, "train_chunk_resample: key_bits=%d unsupported (1..32)", key_bits);
  if (B == 0 || nb_pts == 0) return 0;
  MVK_REQUIRE(row_off && row_len && seeds && sample_rows && sample_pos && (rows || total == 0),
              "train_chunk_resample: null operand");
  hipLaunchKernelGGL(resample_k, dim3(B), dim3(RS_T), 0, (hipStream_t)stream, rows, total, row_off, row_len, seeds, nb_pts,
                     key_bits, sample_rows, sample_pos);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_train_select_frames(const int32_t* bits, int64_t NW, const int64_t* base_point_ind, int64_t NB,
                                       const int64_t* scenes, int S, int64_t P, int64_t F, const int64_t* scene_id,
                                       const int64_t* rows, int64_t total, const int64_t* row_off, const int64_t* row_len,
                                       int B, int nv, int64_t max_base, int64_t max_frames, int32_t* sel, void* stream) {
  MVK_REQUIRE(totals_ok(P, NB, F, NW, S) && total >= 0 && B >= 0 && nv >= 0 && max_base >= 0 && max_frames >= 0 &&
                  total < MAX_SIZE && (int64_t)B * nv < MAX_SIZE,
              "train_select_frames: bad sizes or sizes of 2^31 or more (P=%lld NB=%lld F=%lld NW=%lld S=%d total=%lld B=%d "
              "nv=%d)", (long long)P, (long long)NB, (long long)F, (long long)NW, S, (long long)total, B, nv);
  MVK_REQUIRE(max_base <= MVK_SCENE_MAX_BASE && max_frames <= MVK_SCENE_MAX_FRAMES,
              "train_select_frames: max_base=%lld base points (<= %d: the mask of a chunk's base points is 64 KiB of LDS) or "
              "max_frames=%lld frames (<= %d: their counts live in LDS) exceed the kernel's capacity; there is no fallback",
              (long long)max_base, MVK_SCENE_MAX_BASE, (long long)max_frames, MVK_SCENE_MAX_FRAMES);
  if (B == 0 || nv == 0) return 0;
  MVK_REQUIRE(sel && scenes && scene_id && row_off && row_len && (bits || NW == 0) && (base_point_ind || NB == 0) &&
                  (rows || total == 0),
              "train_select_frames: null operand");
  const int Wmax = (int)cdiv64(max_base, 32);
  const int64_t lds = ((int64_t)Wmax + max_frames) * 4;
  if (lds > 64 * 1024)
    MVK_CHECK_HIP(hipFuncSetAttribute((const void*)train_select_frames_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const Totals tot = {P, NB, F, NW};
  hipLaunchKernelGGL(train_select_frames_k, dim3(B), dim3(SF_T), (size_t)lds, (hipStream_t)stream, (const uint32_t*)bits,
                     base_point_ind, scenes, S, tot, scene_id, rows, total, row_off, row_len, nv, (int)max_base,
                     (int)max_frames, Wmax, sel);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_train_unproject(const int32_t* sel, const int64_t* scene_id, int B, int nv, const int64_t* scenes, int S,
                                   int64_t P, int64_t NB, int64_t F, int64_t NW, const uint16_t* depth,
                                   const float* images_in, const float* poses, const double* cam_inv, int h, int w,
                                   const float* box, const uint8_t* flips, const double* rot, double* keys,
                                   float* image_xyz, uint8_t* image_mask, float* images_out, int32_t* num_valid,
                                   void* stream) {
  MVK_REQUIRE(totals_ok(P, NB, F, NW, S) && B >= 0 && nv >= 0 && h >= 0 && w >= 0,
              "train_unproject: bad sizes (P=%lld NB=%lld F=%lld NW=%lld S=%d B=%d nv=%d h=%d w=%d)", (long long)P,
              (long long)NB, (long long)F, (long long)NW, S, B, nv, h, w);
  const int64_t hw = (int64_t)h * w, Pix = (int64_t)nv * hw;
  const int64_t bpi = cdiv64(Pix, UP_T);
  MVK_REQUIRE(Pix < MAX_SIZE && (hw == 0 || F < MAX_SIZE / hw / 3) && (Pix == 0 || B < MAX_SIZE / Pix / 3) &&
                  (int64_t)B * bpi <= MAX_GRID,
              "train_unproject: sizes of 2^31 or more (B=%d nv=%d F=%lld h=%d w=%d)", B, nv, (long long)F, h, w);
  if (B == 0) return 0;
  MVK_REQUIRE(num_valid, "train_unproject: null operand");
  hipStream_t st = (hipStream_t)stream;
  MVK_CHECK_HIP(hipMemsetAsync(num_valid, 0, (size_t)B * sizeof(int32_t), st));
  if (Pix == 0) return 0;
  MVK_REQUIRE(sel && scene_id && scenes && box && keys && image_xyz && image_mask && images_out &&
                  ((depth && images_in && poses) || F == 0) && (cam_inv || S == 0),
              "train_unproject: null operand");
  const Totals tot = {P, NB, F, NW};
  hipLaunchKernelGGL(train_unproject_k, dim3((unsigned)(B * bpi)), dim3(UP_T), 0, st, sel, scene_id, nv, scenes, S, tot,
                     depth, images_in, poses, cam_inv, h, w, (int)bpi, box, flips, rot, keys, image_xyz, image_mask,
                     images_out, num_valid);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_train_batch_rows(const float* queries, const int64_t* labels, int64_t P, const int64_t* sample_rows,
                                    const double* rot, int B, int64_t nb_pts, float* points_out, int64_t* seg_label,
                                    void* stream) {
  MVK_REQUIRE(P >= 0 && B >= 0 && nb_pts >= 0 && P < MAX_SIZE && nb_pts < MAX_SIZE, "train_batch_rows: bad sizes P=%lld B=%d "
              "nb_pts=%lld", (long long)P, B, (long long)nb_pts);
  const int64_t bpi = cdiv64(nb_pts, BR_T);
  MVK_REQUIRE((nb_pts == 0 || (int64_t)B * 3 < MAX_SIZE / nb_pts) && (int64_t)B * bpi <= MAX_GRID,
              "train_batch_rows: sizes of 2^31 or more (B=%d nb_pts=%lld)", B, (long long)nb_pts);
  if (B == 0 || nb_pts == 0) return 0;
  MVK_REQUIRE(queries && sample_rows && points_out && seg_label && (labels || P == 0), "train_batch_rows: null operand");
  hipLaunchKernelGGL(train_batch_rows_k, dim3((unsigned)(B * bpi)), dim3(BR_T), 0, (hipStream_t)stream, queries, labels, P,
                     sample_rows, rot, (int)bpi, nb_pts, points_out, seg_label);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
