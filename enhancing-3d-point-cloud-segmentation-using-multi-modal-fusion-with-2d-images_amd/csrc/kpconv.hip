// KPConv gather / correlate / aggregate kernels for gfx950 (CDNA4, wave64).
//
// Replaces the ~15 ATen ops of KPConv.forward (reference
// KPConv-PyTorch/models/blocks.py:277-367) and their autograd backward by two
// fused kernels that never materialise [N,H,3], [N,H,K,3], [N,H,K] or [N,H,Cin]:
//
//   gather  (forward)  A[n,k,c]  = sum_h w[n,h,k] * x+[idx[n,h], c]
//   scatter (backward) dx[idx[n,h],c] += sum_k w[n,h,k] * dA[n,k,c]
//
// w[n,h,k] is a pure function of geometry (q, s, kernel points, extent), so the
// backward recomputes it instead of storing [N,H,K].
//
// Work decomposition: see the comment on kpconv_gather_mfma (forward with linear influence and sum aggregation,
// rigid and deformable: one point per wave on the matrix pipe) and kpconv_lane_channel (backward scatter dx, and the
// forward of every other layer: lane = channel, one point per wave, wave-uniform neighbour loop). The offset
// gradient of the deformable layers is csrc/deform.hip (lane = neighbour).
#include <type_traits>

#include "common.h"

#define KMAX 16

namespace {

struct KPParams {
  const float* q;
  const float* s;
  const void* idx;
  const float* x;
  const float* kp;
  const float* offsets;  // [Nq,K,3] or null
  float* min_d2;         // [Nq,K] or null
  int32_t* min_arg;      // [Nq,K] or null: column h of the first entry attaining min_d2 (for the backward)
  float* A;              // fwd: out [Nq,K,Cin]; bwd: in dA
  float* dx;             // bwd out [Ns,Cin]
  const float* g_min_d2; // bwd deformable
  float* d_offsets;      // bwd deformable out [Nq,K,3]
  int64_t Nq, Ns;
  int H, Cin, K;
  float extent;
  int influence, aggregation;
  const int32_t* order;  // MFMA gather (its only reader): work list -- the wave working on slot w takes the point order[w] (a
                         // spatially sorted permutation of 0 .. Nq-1); results land in the points' own rows. null: slot = point
  int xcd_blocks;        // MFMA gather, with `order`: the first xcd_blocks workgroups are dealt to the 8 XCDs as 8 contiguous
                         // runs of the work list
  // MFMA gather, KPM = 2 (gather-form feature gradient of a deformable layer): the kernel points belong to the NEIGHBOUR
  // rows -- nb_offsets [rows of s, K, 3] are added to kp (and the sum is used negated: the relation is transposed) -- and
  // every weight is multiplied by nb_mod [rows of s, K] (modulated layers; null: 1)
  const float* nb_offsets;
  const float* nb_mod;
};

__device__ __forceinline__ float influence_w(float d2, float extent, int influence) {
  // blocks.py:329-344
  if (influence == MVK_INFL_LINEAR) return fmaxf(1.0f - sqrtf(d2) / extent, 0.0f);
  if (influence == MVK_INFL_GAUSSIAN) {
    float sig = extent * 0.3f;
    return expf(-d2 / (2.0f * sig * sig + 1e-9f));
  }
  return 1.0f;
}

__device__ __forceinline__ void wave_sync_lds() {   // LDS hand-off inside ONE wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------
// Phase A of the lane = channel kernel: for the 64 columns h0 .. h0 + 63 of point n's row, fills rel[64] (xyz +
// neighbour row or -1) and w[64][16]. One WAVE works on its own rel / wl (the hand-offs are wave-level: a workgroup may
// hold several independent waves).
// Lane mapping: A1 lane = column h ; A2 item = t*64 + lane, k = lane & 15, column = item >> 4.
// Returns the lane's neighbour row j (A1 mapping).
// ---------------------------------------------------------------------------
template <bool IDX64, bool DEFORM>
__device__ __forceinline__ int phase_a(const KPParams& P, int64_t n, int h0, int lane,
                                       float4* rel, float* wl, float qx, float qy, float qz,
                                       float kx, float ky, float kz,
                                       float* run_min /* DEFORM only */, int* run_arg = nullptr) {
  int j = -2;  // -2: no entry, -1: shadow entry
  float rx = 0.f, ry = 0.f, rz = 0.f;
  if (h0 + lane < P.H) {
    j = load_idx<IDX64>(P.idx, n * P.H + h0 + lane, P.Ns);
    if (j >= 0) {
      const float* sp = P.s + (int64_t)j * 3;
      rx = sp[0] - qx;
      ry = sp[1] - qy;
      rz = sp[2] - qz;
    } else {  // shadow support point (1e6,1e6,1e6), blocks.py:277
      rx = 1e6f - qx;
      ry = 1e6f - qy;
      rz = 1e6f - qz;
    }
  }
  rel[lane] = make_float4(rx, ry, rz, __int_as_float(j));
  wave_sync_lds();

  const int k = lane & 15;
  const float ext2 = P.extent * P.extent;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int ph = t * 4 + (lane >> 4);
    const float4 r = rel[ph];
    const int jj = __float_as_int(r.w);
    float dx = r.x - kx, dy = r.y - ky, dz = r.z - kz;
    float d2 = dx * dx + dy * dy + dz * dz;  // blocks.py:294-297
    float w = 0.f;
    if (jj >= 0 && k < P.K) w = influence_w(d2, P.extent, P.influence);
    if (P.aggregation == MVK_AGG_CLOSEST) {
      // one-hot of argmin_k d2 (first minimum), blocks.py:349-351
      float bd = (k < P.K) ? d2 : INFINITY;
      int bk = k;
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        float od = __shfl_xor(bd, m, 16);
        int ok = __shfl_xor(bk, m, 16);
        if (od < bd || (od == bd && ok < bk)) {
          bd = od;
          bk = ok;
        }
      }
      if (bk != k) w = 0.f;
    }
    if (!DEFORM) {
      // a neighbour on which no kernel point has any influence (beyond the extent of all of them: a third of the real
      // neighbours at conv_radius 2.5 / KP_extent 1.2) contributes exactly nothing: its entry becomes a shadow entry, so
      // the scatter spends no atomics (its bound) and the lane = channel gather no row loads on it
      const unsigned long long mz = __ballot(w != 0.f);
      if (((mz >> (lane & 48)) & 0xFFFFull) == 0ull && k == 0 && jj >= 0) rel[ph].w = __int_as_float(-1);
    }
    if (DEFORM) {
      // neighbours out of range of every deformed kernel point are dropped (blocks.py:306-325)
      unsigned long long m = __ballot(jj >= 0 && k < P.K && d2 < ext2);
      bool inrange = ((m >> (lane & 48)) & 0xFFFFull) != 0ull;
      if (!inrange) {
        w = 0.f;
        if (k == 0 && jj >= 0) rel[ph].w = __int_as_float(-1);
      }
      // running min_h d2 over real + shadow entries (blocks.py:303)
      if (jj >= -1 && k < P.K && d2 < *run_min) {     // strict: this lane visits its entries in ascending h
        *run_min = d2;
        if (run_arg) *run_arg = h0 + ph;
      }
    }
    wl[ph * 16 + k] = w;
  }
  wave_sync_lds();
  return j;
}

// ---------------------------------------------------------------------------
// MFMA gather kernel (round 5; rigid layers, linear influence + sum aggregation, f32): the aggregation
//   A[n, k, c] = sum_h w[n, h, k] x[idx[n, h], c]
// of ONE query point is a [K x H] . [H x Cin] product, and with K = 15 it fits the 16 x 16 x 4 f32 matrix instruction
// exactly: v_mfma_f32_16x16x4_f32 takes A[i][kk] from lane (i = lane & 15, kk = lane >> 4) and B[kk][j] from lane
// (kk = lane >> 4, j = lane & 15) -- so lane (m, kq) computes ONE correlation weight, that of kernel point m for the kq-th
// neighbour of the current group of four, and loads ONE feature value per 16-channel tile, channel m of that neighbour's
// row. No LDS, no phase A / phase B hand-off, no per-neighbour loop of 15 x 4 FMAs per lane: per group of four
// neighbours a wave issues 5 cross-lane reads (the neighbour's row and relative position, read once per 64 columns by the
// lane of that column), ~12 VALU instructions for its weight, T dword loads (16 lanes = 64 contiguous bytes of a row) and
// T MFMAs. The vector kernel it replaced was bound by its own instruction stream (15 x 4 v_pk_fma_f32 per neighbour and lane:
// 57 us for 19 464 x 66 against a 28 us floor of pure FMA issue); here the products run on the matrix
// pipe (exact f32 products, f32 accumulation -- four neighbours per step instead of one: another summation order,
// ~1e-7), 56 MFMAs of 32 cycles per point of that layer = 14 us chip-wide.
// One wave per query point (waves of a workgroup are independent), T accumulator tiles of 16 channels (4 VGPRs each);
// rows wider than 16 T channels run as gridDim.y channel blocks. Work list / XCD runs: KPParams::order, xcd_blocks.
// ---------------------------------------------------------------------------
typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));

// MODE: which channel each lane feeds to tile t -- any assignment works as long as the stores use the same one (column
// j of D depends on column j of B alone), and the texture addresser handles a wave's load at ~16 cycles per instruction
// whatever its width (one CU's addresser serves four matrix pipes), so the loads must be WIDE:
//   1  rows of a multiple of 16 T channels: lane m takes the T consecutive channels c0 + T m .. of its neighbour as
//      8- / 16-byte loads (tile t = its t-th channel): T / 4 load instructions per group instead of T (measured with
//      one dword load per tile: 51 us for 19 464 x 66, 40 us for x 64 -- the addresser, not the matrix pipe, set the pace);
//   2  even rows of 66 .. 80 channels (the early-fusion net's first layer: 64 + 2): channels 4 m .. 4 m + 3 as two
//      8-byte loads (rows are 8-byte aligned) for tiles 0-3, tile 4 = channel 64 + m by a dword load;
//   0  any other row length: tile t = channel c0 + 16 t + m, one dword load per tile.
// KPM: whose kernel points a weight is measured from.
//   0  rigid layer: kernel point m of the layer (P.kp);
//   1  deformable layer, forward (blocks.py:286-327): kernel point m of THIS query point, kp[m] + offsets[n, m] -- one
//      per-lane load per point --, and the layer's second output, min over ALL columns (shadow entries at 1e6 included,
//      blocks.py:303) of the squared distance to each deformed kernel point with the first arg-min column: lane (m, kq)
//      sees columns 4 g + kq in ascending order, the four kq lanes of a kernel point meet at the end. The in-range
//      filter of blocks.py:306-325 needs no code: with the linear influence a neighbour out of range of every kernel
//      point has weight 0 for all of them;
//   2  deformable layer, gather-form feature gradient (the transposed relation: `s` holds the layer's QUERY rows): kernel
//      point m of the NEIGHBOUR row, -(kp[m] + nb_offsets[j, m]), times the modulation nb_mod[j, m] -- two more gathered
//      loads per group, issued with the feature loads.
//
// SW = 4 (launches of few points with long rows: the coarse levels, and every deformable layer -- hundreds of points with
// hundreds of columns at the deform radius): the four waves of a workgroup SHARE one point, wave w takes the group pairs
// w, w + 4, ...; waves 1-3 hand their accumulators (and running minima) to wave 0 through LDS, which adds them in wave
// order (a fixed order) and stores. One wave per point would be a serial chain of H / 4 groups on a fraction of the SIMDs.
template <int T, int MODE, bool IDX64, int KPM = 0, bool SHARE = false>
__global__ __launch_bounds__(256) void kpconv_gather_mfma(KPParams P) {
  static_assert(MODE != 2 || T == 5, "mode 2 is the 64 + tail layout");
  static_assert(MODE != 1 || T == 2 || T % 4 == 0, "mode 1: 8- or 16-byte vectors");
  constexpr int SW = SHARE ? 4 : 1;        // (a template parameter: the one-wave-per-point instantiations keep their registers)
  __shared__ float red_acc[SHARE ? 3 : 1][SHARE ? T * 4 : 1][SHARE ? 64 : 1];
  __shared__ float red_min[SHARE ? 3 : 1][SHARE ? 64 : 1];
  __shared__ int red_arg[SHARE ? 3 : 1][SHARE ? 64 : 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int m = lane & 15, kq = lane >> 4;
  int64_t blk = blockIdx.x;
  if ((int)blockIdx.x < P.xcd_blocks) {      // workgroups go to the XCDs round robin (b % 8): XCD x then works on
    // ONE contiguous run of the sorted work list, so that the rows its L2 pulls are those of one region of the cloud
    const int xq = P.xcd_blocks >> 3, xr = P.xcd_blocks & 7, xc = blockIdx.x & 7;
    blk = (int64_t)xc * xq + min(xc, xr) + (blockIdx.x >> 3);
  }
  const int64_t slot = SW > 1 ? blk : blk * 4 + wid;
  if (slot >= P.Nq) return;                  // (SW 1: the waves of a workgroup never meet; SW 4: the whole workgroup leaves)
  const int gfirst = SW > 1 ? 2 * wid : 0, gstep = 2 * SW;      // this wave's group pairs
  const int n = __builtin_amdgcn_readfirstlane(P.order ? P.order[slot] : (int)slot);
  const int c0 = blockIdx.y * (16 * T);      // first channel of this wave's block
  const float* __restrict__ X = P.x;
  const float qx = P.q[(int64_t)n * 3], qy = P.q[(int64_t)n * 3 + 1], qz = P.q[(int64_t)n * 3 + 2];
  // this lane's kernel point (rows 15.. of the 16-row tile: a point no neighbour is near -> weight 0)
  const int mk = m < P.K ? m : P.K - 1;
  float kx = 1e9f, ky = 1e9f, kz = 1e9f;
  if (m < P.K) {
    kx = P.kp[m * 3];
    ky = P.kp[m * 3 + 1];
    kz = P.kp[m * 3 + 2];
    if (KPM == 1) {
      const float* o = P.offsets + ((int64_t)n * P.K + m) * 3;
      kx += o[0];
      ky += o[1];
      kz += o[2];
    }
  }
  const float inv_ext = 1.0f / P.extent;
  // MODE 0: channel of tile t in this lane, clamped into the row: a lane beyond the row's end loads the last channel again
  // and feeds an output column that is never stored -- no branch, no mask. MODE 1 / 2: first channel of the lane's vector.
  uint32_t chan[MODE == 0 ? T : 1];
  if (MODE == 0) {
#pragma unroll
    for (int t = 0; t < T; ++t) chan[t] = (uint32_t)min(c0 + 16 * t + m, P.Cin - 1);
  } else {
    chan[0] = MODE == 1 ? (uint32_t)(c0 + T * m) : (uint32_t)(4 * m);
  }
  const uint32_t tailc = MODE == 2 ? (uint32_t)min(64 + m, P.Cin - 1) : 0u;
  mfma_f32x4 acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = (mfma_f32x4){0.f, 0.f, 0.f, 0.f};
  float run_min = INFINITY;                  // KPM 1: min over this lane's columns of d2 to kernel point m, first arg-min
  int run_arg = 0x7fffffff;

  for (int h0 = 0; h0 < P.H; h0 += 64) {
    // column h0 + lane of the row: neighbour index (-1: shadow entry, -2: beyond the row), its position relative to the
    // query, the offset of its feature row
    int jl = -2;
    if (h0 + lane < P.H) jl = load_idx<IDX64>(P.idx, (int64_t)n * P.H + h0 + lane, P.Ns);
    float rx = 0.f, ry = 0.f, rz = 0.f;
    if (jl >= 0) {
      const float* sp = P.s + (int64_t)jl * 3;
      rx = sp[0] - qx;
      ry = sp[1] - qy;
      rz = sp[2] - qz;
    } else if (KPM == 1) {                  // shadow support point (1e6, 1e6, 1e6), blocks.py:277: it takes part in min_d2
      rx = 1e6f - qx;
      ry = 1e6f - qy;
      rz = 1e6f - qz;
    }
    const unsigned long long live = __ballot(jl >= 0);
    if (KPM != 1 && live == 0ull) continue;
    // KPM 1 walks every column of the row (the shadow entries count for min_d2), the others stop at the last real entry
    const int ncol = min(64, P.H - h0);
    const int groups = KPM == 1 ? (ncol + 3) >> 2 : (64 - __builtin_clzll(live) + 3) >> 2;        // wave-uniform
    const uint32_t roff = (uint32_t)(jl >= 0 ? jl : 0) * (uint32_t)P.Cin;      // (host: Ns * Cin < 2^32)
    // Group g: lane (m, kq) works on column 4 g + kq. Two register sets, the loop unrolled by two: the cross-lane reads
    // and the feature loads of the NEXT group are issued before the MFMAs of the current one, nothing in the body is
    // conditional (a branch around a load makes the compiler wait for everything in flight). A group beyond `groups`
    // (odd counts; columns >= 64 wrap around in the cross-lane read) has weight 0: its columns are shadow entries.
    auto fetch = [&](const int g, float& w, float (&xv)[T]) {
      const int src = 4 * g + kq;
      const int j = __shfl(jl, src);
      float gx = __shfl(rx, src), gy = __shfl(ry, src), gz = __shfl(rz, src);
      const uint32_t off = (uint32_t)__shfl((int)roff, src);
      float wmod = 1.0f;
      if (KPM == 2) {
        // the neighbour row's own kernel point m (clamped indices: the loads are unconditional), used negated
        const int jr = j >= 0 ? j : 0;
        const float* o = P.nb_offsets + ((int64_t)jr * P.K + mk) * 3;
        gx += kx + o[0];
        gy += ky + o[1];
        gz += kz + o[2];
        if (P.nb_mod) wmod = P.nb_mod[(int64_t)jr * P.K + mk];
      } else {
        gx -= kx;
        gy -= ky;
        gz -= kz;
      }
      const float d2 = gx * gx + gy * gy + gz * gz;                                  // blocks.py:294-297
      const float d = __builtin_amdgcn_sqrtf(d2);                                    // :333-335
      w = (j >= 0 && src < 64) ? fmaxf(1.0f - d * inv_ext, 0.0f) * wmod : 0.0f;
      if (KPM == 1 && j >= -1 && src < 64 && m < P.K && d2 < run_min) {             // ascending columns: strict <
        run_min = d2;
        run_arg = h0 + src;
      }
      if (MODE == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) xv[t] = X[off + chan[t]];
      } else if (MODE == 1 && T == 2) {
        const float2 v = *reinterpret_cast<const float2*>(X + off + chan[0]);
        xv[0] = v.x;
        xv[1] = v.y;
      } else if (MODE == 1) {
#pragma unroll
        for (int u = 0; u < T / 4; ++u) {
          const float4 v = *reinterpret_cast<const float4*>(X + off + chan[0] + 4 * u);
          xv[4 * u] = v.x;
          xv[4 * u + 1] = v.y;
          xv[4 * u + 2] = v.z;
          xv[4 * u + 3] = v.w;
        }
      } else {
        const float2 v0 = *reinterpret_cast<const float2*>(X + off + chan[0]);
        const float2 v1 = *reinterpret_cast<const float2*>(X + off + chan[0] + 2);
        xv[0] = v0.x;
        xv[1] = v0.y;
        xv[2] = v1.x;
        xv[3] = v1.y;
        xv[T - 1] = X[off + tailc];
      }
    };
    float wa, wb;
    float xa[T], xb[T];
    // (KPM 1: a group is fetched exactly once -- fetch also updates the running minimum -- so the look-ahead stops at
    // the last group; the other modes may fetch one group past the end, whose weights are zero)
    if (gfirst >= groups) continue;
    fetch(gfirst, wa, xa);
    for (int g = gfirst; g < groups; g += gstep) {
      if (KPM != 1 || g + 1 < groups) fetch(g + 1, wb, xb);
      else wb = 0.0f;
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa, xa[t], acc[t], 0, 0, 0);
      if (KPM != 1 || g + gstep < groups) fetch(g + gstep, wa, xa);
      if (KPM != 1 || g + 1 < groups) {
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb, xb[t], acc[t], 0, 0, 0);
      }
    }
  }
  if (SHARE) {
    // waves 1 .. 3 park their partial results, wave 0 adds them in wave order
    if (wid > 0) {
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red_acc[wid - 1][t * 4 + r][lane] = acc[t][r];
      red_min[wid - 1][lane] = run_min;
      red_arg[wid - 1][lane] = run_arg;
    }
    __syncthreads();
    if (wid > 0) return;
    for (int w = 0; w < SW - 1; ++w) {
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] += red_acc[w][t * 4 + r][lane];
      const float od = red_min[w][lane];
      const int oa = red_arg[w][lane];
      if (od < run_min || (od == run_min && oa < run_arg)) {
        run_min = od;
        run_arg = oa;
      }
    }
  }
  if (KPM == 1 && P.min_d2 != nullptr && blockIdx.y == 0) {
    // the four column residues of kernel point m: smaller distance wins, equal distances the smaller column (the FIRST
    // arg-min over all columns, like a sequential scan)
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float od = __shfl_xor(run_min, o);
      const int oa = __shfl_xor(run_arg, o);
      if (od < run_min || (od == run_min && oa < run_arg)) {
        run_min = od;
        run_arg = oa;
      }
    }
    if (kq == 0 && m < P.K) {
      P.min_d2[(int64_t)n * P.K + m] = run_min;
      if (P.min_arg) P.min_arg[(int64_t)n * P.K + m] = run_arg;
    }
  }
  // D[i][j]: lane (j = m, i = 4 kq + r) holds kernel point 4 kq + r in register r of tile t, i.e. of the channel the lane
  // fed to tile t
  float* __restrict__ out = P.A + (int64_t)n * P.K * P.Cin;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kpt = 4 * kq + r;
    if (kpt >= P.K) continue;
    float* __restrict__ o = out + (int64_t)kpt * P.Cin;
    if (MODE == 0) {
#pragma unroll
      for (int t = 0; t < T; ++t)
        if (c0 + 16 * t + m < P.Cin) o[c0 + 16 * t + m] = acc[t][r];
    } else if (MODE == 1 && T == 2) {
      *reinterpret_cast<float2*>(o + c0 + 2 * m) = make_float2(acc[0][r], acc[1][r]);
    } else if (MODE == 1) {
#pragma unroll
      for (int u = 0; u < T / 4; ++u)
        *reinterpret_cast<float4*>(o + c0 + T * m + 4 * u) =
            make_float4(acc[4 * u][r], acc[4 * u + 1][r], acc[4 * u + 2][r], acc[4 * u + 3][r]);
    } else {
      *reinterpret_cast<float2*>(o + 4 * m) = make_float2(acc[0][r], acc[1][r]);
      *reinterpret_cast<float2*>(o + 4 * m + 2) = make_float2(acc[2][r], acc[3][r]);
      if (64 + m < P.Cin) o[64 + m] = acc[T - 1][r];
    }
  }
}

// ---------------------------------------------------------------------------
// Generic lane = channel kernel (one point per wave). MODE 0: forward of every layer the MFMA gather does not take
// (any influence, aggregation, Cin and table size, rigid or deformable). MODE 1: backward scatter (+ deformable grads).
// Channels handled: c = c0 + lane + 64*slot, slot < NSLOT.
// ---------------------------------------------------------------------------
// WPB > 1 (backward scatter of the layers searched at the deform radius: hundreds of neighbour columns for a few
// hundred points): the WPB waves of a workgroup work on the SAME point, wave w on the 64-neighbour chunks w, w + WPB,
// ...; they meet only in the atomics on dx (one wave per point was a 26 us serial chain on a third of the SIMDs).
// HS > 1 (scatter of the coarse levels, a few hundred points or fewer: one wave per point leaves most SIMDs idle behind
// a serial chain of H neighbours x NSLOT atomics): the workgroup's HS waves all evaluate the chunk's weights and take
// every HS-th neighbour each, and the 64-channel slots of a point are spread over blockIdx.y (NSLOT = 1) -- level 4
// (85 points, 512 channels): 85 waves -> 2 720.
template <int NSLOT, bool IDX64, int MODE, bool DEFORM, int WPB = 1, int HS = 1>
__global__ __launch_bounds__(64 * WPB * HS) void kpconv_lane_channel(KPParams P, int c0_base) {
  constexpr int HC = 64;
  static_assert(WPB == 1 || MODE == 1, "only the scatter splits a point over waves");
  static_assert(HS == 1 || (MODE == 1 && WPB == 1 && !DEFORM), "neighbour interleave: rigid scatter only");
  const int c0 = c0_base + (int)blockIdx.y * 64 * NSLOT;
  __shared__ float4 rel_all[WPB * HS][64];
  __shared__ float wl_all[WPB * HS][64 * 16];
  const int lane = threadIdx.x & 63, wid_all = threadIdx.x >> 6;
  const int wid = HS > 1 ? 0 : wid_all;          // HS: every wave walks all chunks
  float4* rel = rel_all[wid_all];
  float* wl = wl_all[wid_all];
  const int64_t n = blockIdx.x;
  const float* qp = P.q + n * 3;
  const float qx = qp[0], qy = qp[1], qz = qp[2];
  const int k = lane & 15;
  float kx = 0.f, ky = 0.f, kz = 0.f;
  if (k < P.K) {
    kx = P.kp[k * 3];
    ky = P.kp[k * 3 + 1];
    kz = P.kp[k * 3 + 2];
    if (DEFORM) {  // deformed kernel point (blocks.py:287)
      const float* o = P.offsets + (n * P.K + k) * 3;
      kx += o[0];
      ky += o[1];
      kz += o[2];
    }
  }
  float run_min = INFINITY;
  int run_arg = 0;

  float acc[NSLOT][KMAX - 1];  // MODE 0: A accumulators; MODE 1: dA values
#pragma unroll
  for (int sidx = 0; sidx < NSLOT; ++sidx) {
    const int c = c0 + lane + 64 * sidx;
#pragma unroll
    for (int kk = 0; kk < KMAX - 1; ++kk) {
      if (MODE == 0)
        acc[sidx][kk] = 0.f;
      else
        acc[sidx][kk] = (c < P.Cin && kk < P.K) ? P.A[(n * P.K + kk) * P.Cin + c] : 0.f;
    }
  }

  for (int h0 = wid * HC; h0 < P.H; h0 += HC * WPB) {
    int j = phase_a<IDX64, DEFORM>(P, n, h0, lane, rel, wl, qx, qy, qz, kx, ky, kz, &run_min, &run_arg);
    if (__ballot(j >= 0) != 0ull) {
      const int hend = min(HC, P.H - h0);
      for (int hh = HS > 1 ? wid_all : 0; hh < hend; hh += HS) {
        const int jj = __builtin_amdgcn_readfirstlane(__float_as_int(rel[hh].w));
        if (jj < 0) continue;  // wave-uniform
        const float4* w4 = reinterpret_cast<const float4*>(wl + hh * 16);
        const float4 wa = w4[0], wb = w4[1], wc = w4[2], wd = w4[3];
        const float wv[16] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w,
                              wc.x, wc.y, wc.z, wc.w, wd.x, wd.y, wd.z, wd.w};
#pragma unroll
        for (int sidx = 0; sidx < NSLOT; ++sidx) {
          const int c = c0 + lane + 64 * sidx;
          if (c < P.Cin) {
            if (MODE == 0) {
              const float xv = P.x[(int64_t)jj * P.Cin + c];
#pragma unroll
              for (int kk = 0; kk < KMAX - 1; ++kk) acc[sidx][kk] += wv[kk] * xv;
            } else {
              float contrib = 0.f;
#pragma unroll
              for (int kk = 0; kk < KMAX - 1; ++kk) contrib += wv[kk] * acc[sidx][kk];
              atomicAdd(P.dx + (int64_t)jj * P.Cin + c, contrib);
            }
          }
        }
      }
    }
    wave_sync_lds();
  }

  if (MODE == 0) {
#pragma unroll
    for (int sidx = 0; sidx < NSLOT; ++sidx) {
      const int c = c0 + lane + 64 * sidx;
      if (c < P.Cin) {
#pragma unroll
        for (int kk = 0; kk < KMAX - 1; ++kk)
          if (kk < P.K) P.A[(n * P.K + kk) * P.Cin + c] = acc[sidx][kk];
      }
    }
    if (DEFORM && P.min_d2 != nullptr && c0 == 0) {
      float m = run_min;      // lanes l, l^16, l^32, l^48 hold kernel point k = l & 15: (value, column) minimum, first column on ties
      int a = run_arg;
#pragma unroll
      for (int sh = 16; sh <= 32; sh <<= 1) {
        const float om = __shfl_xor(m, sh);
        const int oa = __shfl_xor(a, sh);
        if (om < m || (om == m && oa < a)) {
          m = om;
          a = oa;
        }
      }
      if (lane < 16 && lane < P.K) {
        P.min_d2[n * P.K + lane] = m;
        if (P.min_arg) P.min_arg[n * P.K + lane] = a;
      }
    }
  }
}

// channel tiles per wave of the MFMA gather for rows of Cin channels (0: the lane = channel kernel)
int mfma_tiles(int64_t Ns, int Cin, int K, int influence, int aggregation) {
  if (influence != MVK_INFL_LINEAR || aggregation != MVK_AGG_SUM || K > 16 || Cin < 1) return 0;
  if ((uint64_t)Ns * (uint64_t)Cin >= (1ull << 32) - 4096) return 0;
  if (Cin <= 32) return 2;
  if (Cin <= 64) return 4;
  if (Cin <= 80) return 5;            // 66: the early-fusion net's first layer
  if (Cin <= 128) return 8;
  return 16;                          // wider rows: gridDim.y blocks of 256 channels
}

// launch shape of the MFMA gather (shared by the launch and by mvk_kpconv_gather_plan): T = 0: not on this kernel
struct MfmaPlan {
  int T, SW;               // accumulator tiles per wave; waves sharing one point (1 or 4)
  int64_t wgs, blocks_y;   // grid
};
MfmaPlan plan_mfma(int64_t Nq, int64_t Ns, int H, int Cin, int K, int influence, int aggregation, bool deform) {
  MfmaPlan m{};
  m.T = mfma_tiles(Ns, Cin, K, influence, aggregation);
  if (m.T == 0) return m;
  // few points with long rows: the four waves of a workgroup share one point (kernel comment)
  m.blocks_y = cdiv64(Cin, 16 * m.T);
  const bool can_share = m.T >= 4 && m.T != 5;          // (instantiated for the tile counts the coarse levels use)
  m.SW = (can_share && (H >= 128 || (Nq * m.blocks_y <= 512 && H >= 32))) ? 4 : 1;
  m.wgs = m.SW > 1 ? Nq : cdiv64(Nq, 4);
  return m;
}

template <int KPM>
bool launch_mfma(KPParams P, int idx64, hipStream_t st) {
  const MfmaPlan mp = plan_mfma(P.Nq, P.Ns, P.H, P.Cin, P.K, P.influence, P.aggregation, KPM == 1);
  const int T = mp.T;
  if (T == 0) return false;
  const int SW = mp.SW;
  const int64_t wgs = mp.wgs;
  P.xcd_blocks = P.order != nullptr ? (int)wgs : 0;
  dim3 grid((unsigned)wgs, (unsigned)mp.blocks_y), block(256);
#define LM1(TT, MD, SH)                                                                              \
  if (idx64) hipLaunchKernelGGL((kpconv_gather_mfma<TT, MD, true, KPM, SH>), grid, block, 0, st, P);     \
  else hipLaunchKernelGGL((kpconv_gather_mfma<TT, MD, false, KPM, SH>), grid, block, 0, st, P)
#define LM(TT, MD)                                          \
  if (SW > 1 && TT >= 4 && TT != 5) { LM1(TT, MD, (TT >= 4 && TT != 5)); } else { LM1(TT, MD, false); }
  // wide loads where the row length allows them (kernel comment): rows of a multiple of 16 T channels from a 16-byte
  // aligned table; the 64 + tail layout for even rows of 66 .. 80 channels; one dword per tile otherwise
  const bool wide = P.Cin % (16 * T) == 0 && ((uintptr_t)P.x & 15) == 0 && ((uintptr_t)P.A & 15) == 0;
  const bool tail5 = T == 5 && P.Cin > 64 && P.Cin % 2 == 0 && ((uintptr_t)P.x & 7) == 0 && ((uintptr_t)P.A & 7) == 0;
  if (T == 2) { if (wide) { LM(2, 1); } else { LM(2, 0); } }
  else if (T == 4) { if (wide) { LM(4, 1); } else { LM(4, 0); } }
  else if (T == 5) { if (tail5 && KPM == 0) { LM(5, 2); } else { LM(5, 0); } }
  else if (T == 8) { if (wide) { LM(8, 1); } else { LM(8, 0); } }
  else { if (wide) { LM(16, 1); } else { LM(16, 0); } }
#undef LM1
#undef LM
  return true;
}

template <int MODE, bool DEFORM>
int launch_lane_channel(const KPParams& P, int idx64, hipStream_t st) {
  // scatter of a layer with more than one 64-neighbour chunk (searched at the deform radius): four waves per point
  const bool split = MODE == 1 && P.H > 64;
  if (MODE == 1 && !DEFORM && !split && P.Nq < 2048) {
    // few points (coarse levels): one wave per (point, 64-channel slot), and below ~4 000 such waves four waves per
    // slot that take every fourth neighbour (see the kernel's HS parameter)
    const int slots = (P.Cin + 63) / 64;
    const bool hs = (int64_t)P.Nq * slots < 4096;
    dim3 grid((unsigned)P.Nq, (unsigned)slots), block(hs ? 256 : 64);
    if (hs) {
      if (idx64) hipLaunchKernelGGL((kpconv_lane_channel<1, true, 1, false, 1, 4>), grid, block, 0, st, P, 0);
      else hipLaunchKernelGGL((kpconv_lane_channel<1, false, 1, false, 1, 4>), grid, block, 0, st, P, 0);
    } else {
      if (idx64) hipLaunchKernelGGL((kpconv_lane_channel<1, true, 1, false, 1, 1>), grid, block, 0, st, P, 0);
      else hipLaunchKernelGGL((kpconv_lane_channel<1, false, 1, false, 1, 1>), grid, block, 0, st, P, 0);
    }
    return 0;
  }
  dim3 grid((unsigned)P.Nq), block(split ? 256 : 64);
  for (int c0 = 0; c0 < P.Cin; c0 += 512) {
    int cw = P.Cin - c0 < 512 ? P.Cin - c0 : 512;
    int ns = (cw + 63) / 64;
#define LC(NS)                                                                                       \
  if (split) {                                                                                       \
    if (idx64)                                                                                       \
      hipLaunchKernelGGL((kpconv_lane_channel<NS, true, MODE, DEFORM, (MODE == 1 ? 4 : 1)>), grid, block, 0, st, P, c0);  \
    else                                                                                             \
      hipLaunchKernelGGL((kpconv_lane_channel<NS, false, MODE, DEFORM, (MODE == 1 ? 4 : 1)>), grid, block, 0, st, P, c0); \
  } else if (idx64)                                                                                  \
    hipLaunchKernelGGL((kpconv_lane_channel<NS, true, MODE, DEFORM>), grid, block, 0, st, P, c0);    \
  else                                                                                               \
    hipLaunchKernelGGL((kpconv_lane_channel<NS, false, MODE, DEFORM>), grid, block, 0, st, P, c0);
    if (ns <= 1) {
      LC(1)
    } else if (ns <= 2) {
      LC(2)
    } else if (ns <= 4) {
      LC(4)
    } else {
      LC(8)
    }
#undef LC
  }
  return 0;
}

int check_common(int64_t Nq, int64_t Ns, int H, int Cin, int K, int influence, int aggregation) {
  MVK_REQUIRE(Nq >= 0 && Ns >= 0 && H >= 0 && Cin > 0, "kpconv: bad sizes Nq=%lld Ns=%lld H=%d Cin=%d",
              (long long)Nq, (long long)Ns, H, Cin);
  MVK_REQUIRE(K >= 1 && K < KMAX, "kpconv: kernel size K=%d unsupported (1..%d)", K, KMAX - 1);
  MVK_REQUIRE(influence >= 0 && influence <= 2, "Unknown influence function type (config.KP_influence)");
  MVK_REQUIRE(aggregation == 0 || aggregation == 1, "Unknown convolution mode. Should be 'closest' or 'sum'");
  MVK_REQUIRE(Nq < (1ll << 31), "kpconv: Nq too large for one launch");
  return 0;
}

}  // namespace

extern "C" int mvk_kpconv_gather_fwd(const float* q, int64_t Nq, const float* s, int64_t Ns,
                                     const void* idx, int idx64, int H, const float* x, int Cin,
                                     const float* kp, int K, float extent, int influence,
                                     int aggregation, const float* offsets, float* min_d2,
                                     int32_t* min_arg, float* A_out, void* stream) {
  return mvk_kpconv_gather_fwd_ordered(q, Nq, s, Ns, idx, idx64, H, x, Cin, kp, K, extent, influence, aggregation, offsets,
                                       min_d2, min_arg, A_out, nullptr, stream);
}

extern "C" int mvk_kpconv_gather_fwd_ordered(const float* q, int64_t Nq, const float* s, int64_t Ns,
                                             const void* idx, int idx64, int H, const float* x, int Cin,
                                             const float* kp, int K, float extent, int influence,
                                             int aggregation, const float* offsets, float* min_d2,
                                             int32_t* min_arg, float* A_out, const int32_t* order, void* stream) {
  if (int e = check_common(Nq, Ns, H, Cin, K, influence, aggregation)) return e;
  if (Nq == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  KPParams P{};
  P.order = order;        // read by the MFMA gather; the lane = channel kernel works in row order
  P.q = q; P.s = s; P.idx = idx; P.x = x; P.kp = kp; P.offsets = offsets; P.min_d2 = min_d2; P.min_arg = min_arg;
  P.A = A_out; P.Nq = Nq; P.Ns = Ns; P.H = H; P.Cin = Cin; P.K = K; P.extent = extent;
  P.influence = influence; P.aggregation = aggregation;
  if (H == 0) {
    MVK_CHECK_HIP(hipMemsetAsync(A_out, 0, sizeof(float) * Nq * K * Cin, st));
    if (offsets == nullptr) return 0;
  }
  // the aggregation on the matrix pipe (linear influence, sum aggregation, feature table < 2^32 elements), everything
  // else one point per wave with lane = channel
  if (offsets != nullptr) {
    KPParams Pm = P;
    Pm.order = nullptr;           // (the deformable levels are the coarse ones: no work list)
    if (!launch_mfma<1>(Pm, idx64, st)) launch_lane_channel<0, true>(P, idx64, st);
  } else if (!launch_mfma<0>(P, idx64, st)) {
    launch_lane_channel<0, false>(P, idx64, st);
  }
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

// Gather-form feature gradient of a DEFORMABLE KPConv (round 5; blocks.py:286-327, :360 through autograd). With the
// transposed neighbourhood relation rev [Ns, Hr] (row j = the query rows n whose list holds support j; entries outside
// [0, Nq) are shadow entries), g [Nq, C] the gradient of the layer's output and the layer's own deformed kernel points
// kp [K, 3] + offsets [Nq, K, 3] and modulations mod [Nq, K] (null: not modulated):
//   A2 [Ns, K, C] [j, k, :] = sum over n in rev[j] of max(0, 1 - |s_j - q_n - kp_k - offsets[n, k]| / extent) mod[n, k] g[n, :]
// i.e. the forward aggregation over the transposed relation with the kernel points of the NEIGHBOUR rows; the feature
// gradient is then dx = sum_k A2[:, k, :] . W[k]^T (mvk_gemm_f32_kp_transposed) -- no atomics, a fixed summation order per
// row of rev. Linear influence, sum aggregation, 5 <= C, Nq * C < 2^32 (returns an error otherwise: the caller keeps
// mvk_kpconv_scatter_bwd). order: a work list over the Ns rows or NULL.
extern "C" int mvk_kpconv_gather_rev_deform(const float* s, int64_t Ns, const float* q, int64_t Nq, const void* rev, int rev64,
                                            int Hr, const float* g, int C, const float* kp, int K, float extent,
                                            const float* offsets, const float* mod, float* A2, const int32_t* order,
                                            void* stream) {
  if (int e = check_common(Ns, Nq, Hr, C, K, MVK_INFL_LINEAR, MVK_AGG_SUM)) return e;
  MVK_REQUIRE(offsets != nullptr && A2 != nullptr, "kpconv rev deform: offsets and an output are required");
  if (Ns == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (Hr == 0 || Nq == 0) {
    MVK_CHECK_HIP(hipMemsetAsync(A2, 0, sizeof(float) * Ns * K * C, st));
    return 0;
  }
  KPParams P{};
  // roles transposed: the "queries" of the launch are the layer's supports, its "supports" the layer's query rows
  P.q = s; P.s = q; P.idx = rev; P.x = g; P.kp = kp; P.A = A2; P.Nq = Ns; P.Ns = Nq; P.H = Hr; P.Cin = C; P.K = K;
  P.extent = extent; P.influence = MVK_INFL_LINEAR; P.aggregation = MVK_AGG_SUM;
  P.order = order; P.nb_offsets = offsets; P.nb_mod = mod;
  MVK_REQUIRE(launch_mfma<2>(P, rev64, st), "kpconv rev deform: shape not supported by the MFMA gather (C >= 5, Nq * C < 2^32)");
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_kpconv_scatter_bwd(const float* q, int64_t Nq, const float* s, int64_t Ns,
                                      const void* idx, int idx64, int H, int Cin, const float* kp,
                                      int K, float extent, int influence, int aggregation,
                                      const float* dA, float* dx, const float* x,
                                      const float* offsets, const float* g_min_d2, const int32_t* min_arg,
                                      float* d_offsets, void* stream) {
  if (int e = check_common(Nq, Ns, H, Cin, K, influence, aggregation)) return e;
  if (Nq == 0 || H == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  KPParams P{};
  P.q = q; P.s = s; P.idx = idx; P.x = x; P.kp = kp; P.offsets = offsets;
  P.A = const_cast<float*>(dA); P.dx = dx; P.g_min_d2 = g_min_d2; P.d_offsets = d_offsets;
  P.Nq = Nq; P.Ns = Ns; P.H = H; P.Cin = Cin; P.K = K; P.extent = extent;
  P.influence = influence; P.aggregation = aggregation;
  if (offsets != nullptr) {
    MVK_REQUIRE(x != nullptr && d_offsets != nullptr, "kpconv bwd: deformable needs x and d_offsets");
    MVK_REQUIRE(aggregation == MVK_AGG_SUM, "kpconv bwd: deformable + 'closest' aggregation has no offset gradient path");
    launch_lane_channel<1, true>(P, idx64, st);      // dx: same scatter as the rigid layers, deformed weights + in-range filter
    MVK_CHECK_HIP(hipGetLastError());
    // d_offsets (A path and min_d2 path): one wave per point, lane = neighbour (csrc/deform.hip)
    return mvk_kpconv_deform_doff(q, Nq, s, Ns, idx, idx64, H, x, Cin, kp, K, extent, influence, offsets, dA, g_min_d2,
                                  min_arg, d_offsets, stream);
  } else {
    launch_lane_channel<1, false>(P, idx64, st);
  }
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

// Launch geometry mvk_kpconv_gather_fwd uses for a layer (elem_bytes: 4, the f32 rows -- the only row type)
// with linear influence and sum aggregation. On the MFMA gather out[0..7] = 64 (lanes per point), 1 (point per wave),
// channel tiles per wave, 0 (the four waves of a workgroup share one point) or -1 (one point each), 4 (waves per
// workgroup), workgroups, grid threads (what a kernel trace reports), 1. All eight are 0 when the layer runs on the
// lane = channel kernel (one point per wave) or launches nothing.
extern "C" int mvk_kpconv_gather_plan(int64_t Nq, int64_t Ns, int H, int Cin, int elem_bytes, int deformable,
                                      int64_t* out) {
  MVK_REQUIRE(out != nullptr && elem_bytes == 4, "kpconv plan: bad arguments (feature rows are f32: elem_bytes 4)");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  const MfmaPlan mp = plan_mfma(Nq, Ns, H, Cin, 15, MVK_INFL_LINEAR, MVK_AGG_SUM, deformable != 0);
  if (Nq > 0 && mp.T > 0) {        // four waves per workgroup (one point each, or sharing one), channel blocks in gridDim.y
    out[0] = 64; out[1] = 1; out[2] = mp.T; out[3] = mp.SW > 1 ? 0 : -1; out[4] = 4; out[5] = mp.wgs * mp.blocks_y;
    out[6] = out[5] * 256; out[7] = 1;
  }
  return 0;
}
