// The exact float64 k-NN's arithmetic, shared by mvk_knn_f64 (csrc/fusion.hip) and mvk_knn_f64_ragged
// (csrc/sphere_inputs.hip) so that the two cannot differ: the distance expression, the (d2, index)-ordered top-k
// insertion, the Morton grid that orders queries and keys, and the pruned search of one workgroup over the 64-key
// tiles of one key set. Include from a translation unit compiled with -ffp-contract=off.
#pragma once
#include "common.h"

// squared distance in three rounded products and three rounded sums, in this order
__device__ __forceinline__ double knn_d2(double qx, double qy, double qz, double x, double y, double z) {
  const double dx = qx - x, dy = qy - y, dz = qz - z;
  double d2 = 0.0;
  d2 += dx * dx;
  d2 += dy * dy;
  d2 += dz * dz;
  return d2;
}

// keeps bd / bi sorted by (d2, index); I is int64_t or int
template <int K, typename I>
__device__ __forceinline__ void topk_insert(double (&bd)[K], I (&bi)[K], double d2, I j) {
  if (d2 < bd[K - 1] || (d2 == bd[K - 1] && j < bi[K - 1])) {
    bd[K - 1] = d2;
    bi[K - 1] = j;
#pragma unroll
    for (int p = K - 1; p > 0; --p) {
      if (bd[p] < bd[p - 1] || (bd[p] == bd[p - 1] && bi[p] < bi[p - 1])) {
        const double td = bd[p]; bd[p] = bd[p - 1]; bd[p - 1] = td;
        const I ti = bi[p]; bi[p] = bi[p - 1]; bi[p - 1] = ti;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Pruned exact k-NN (same results as brute force, bit for bit):
//   1. queries and valid keys are binned into a 32^3 Morton-ordered torus grid (cell 0.1 m; the
//      binning only decides the ORDER things are visited in, never the result), counting sort;
//   2. every run of 64 sorted keys is a tile with an axis-aligned box (float, rounded outwards);
//   3. a workgroup owns 64 consecutive sorted queries (a compact patch). Per query an upper bound of
//      the k-th distance follows from the boxes alone (ub = min over tiles holding >= k keys of the
//      farthest box corner); a tile is visited only if some query of the wave has
//      min-dist(box) <= min(ub, its current k-th best). Every key with d2 <= the true k-th distance
//      sits in such a tile, ties included, so the (d2, index)-ordered top-k is the brute-force one.
//      The waves of the workgroup share out the candidate tiles and merge their results in LDS.
// ---------------------------------------------------------------------------------------------
constexpr int PG = 32, PNC = PG * PG * PG;        // grid cells
constexpr float PCELL_INV = 10.f;                  // 1 / 0.1 m
constexpr int PT = 64;                             // keys per tile
constexpr int PCH = 1024;                          // tiles considered at a time (candidate list <= 36 KB of LDS)

__device__ __forceinline__ unsigned spread3(unsigned v) {  // 5 bits -> every third bit
  v &= 31u;
  v = (v | (v << 8)) & 0x0000100Fu;
  v = (v | (v << 4)) & 0x000010C3u;
  v = (v | (v << 2)) & 0x00001249u;
  return v;
}
__device__ __forceinline__ int morton_cell(float x, float y, float z) {
  const int ix = (int)floorf(x * PCELL_INV), iy = (int)floorf(y * PCELL_INV), iz = (int)floorf(z * PCELL_INV);
  return (int)(spread3((unsigned)ix) | (spread3((unsigned)iy) << 1) | (spread3((unsigned)iz) << 2));
}

// exclusive scan of PNC cell counts by one workgroup of 1024 threads x 32 cells; returns the total to every thread
__device__ __forceinline__ int pk_scan_cells(const int* __restrict__ cnt, int* __restrict__ start) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  constexpr int PER = PNC / 1024;
  int loc[PER], s = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    loc[i] = s;
    s += cnt[tid * PER + i];
  }
  part[tid] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const int base = part[tid] - s;
#pragma unroll
  for (int i = 0; i < PER; ++i) start[tid * PER + i] = base + loc[i];
  return part[1023];
}

// one wave: the outward-rounded float box of tile t of nv sorted keys -> b[0..7] = lo xyz, hi xyz, count, pad
__device__ __forceinline__ void pk_tile_box(const double* __restrict__ skey, int nv, int t, float* __restrict__ b) {
  const int p = t * PT + threadIdx.x;
  if (t * PT >= nv) {
    if (threadIdx.x == 0) b[6] = 0.f;
    return;
  }
  const bool ok = p < nv;
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = ok ? skey[(int64_t)p * 3 + a] : 0.0;
    lo[a] = ok ? __double2float_rd(v) : INFINITY;
    hi[a] = ok ? __double2float_ru(v) : -INFINITY;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
    }
  }
  if (threadIdx.x == 0) {
    b[0] = lo[0]; b[1] = lo[1]; b[2] = lo[2];
    b[3] = hi[0]; b[4] = hi[1]; b[5] = hi[2];
    b[6] = (float)min(PT, nv - t * PT);
  }
}

// The search of one workgroup of PW waves: lane l of every wave holds the same query (q[qi], when live) and the waves
// share out the tiles of ONE key set: box [ntiles][8], skey [nv][3] sorted keys, sidx [nv] their original numbers.
// Writes out[qi * kout + c], c < kout (-1 where fewer than c + 1 keys exist). Every thread of the workgroup must call it.
template <int K, int PW>
__device__ __forceinline__ void knn_pruned_search(const float* __restrict__ q, bool live, int64_t qi,
                                                  const float* __restrict__ box, const double* __restrict__ skey,
                                                  const int* __restrict__ sidx, int nv, int ntiles_max, int kout,
                                                  int64_t* __restrict__ out) {
  __shared__ double sk[PW][3][PT];
  __shared__ int si[PW][PT];
  __shared__ float sub[PW][64];
  // candidate list during the sweeps, merge buffers afterwards (same LDS bytes)
  constexpr int CAND_BYTES = PCH * 36, MERGE_BYTES = PW * 64 * K * 12;
  __shared__ __attribute__((aligned(16))) char un[CAND_BYTES > MERGE_BYTES ? CAND_BYTES : MERGE_BYTES];
  float4 (*cbox)[2] = reinterpret_cast<float4 (*)[2]>(un);          // [PCH][2] boxes of the candidate tiles
  int* cand = reinterpret_cast<int*>(un + PCH * 32);                 // [PCH] their tile ids
  double (*md)[64][K] = reinterpret_cast<double (*)[64][K]>(un);      // [PW][64][K]
  int (*mi)[64][K] = reinterpret_cast<int (*)[64][K]>(un + PW * 64 * K * 8);
  __shared__ int ncand;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float fx = live ? q[qi * 3] : 0.f, fy = live ? q[qi * 3 + 1] : 0.f, fz = live ? q[qi * 3 + 2] : 0.f;
  const double qx = fx, qy = fy, qz = fz;
  const int ntiles = min(ntiles_max, (nv + PT - 1) / PT);

  // box of the workgroup's 64 queries (every wave holds the same queries)
  float ql[3] = {live ? fx : INFINITY, live ? fy : INFINITY, live ? fz : INFINITY};
  float qh[3] = {live ? fx : -INFINITY, live ? fy : -INFINITY, live ? fz : -INFINITY};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      ql[a] = fminf(ql[a], __shfl_xor(ql[a], off));
      qh[a] = fmaxf(qh[a], __shfl_xor(qh[a], off));
    }

  // A. workgroup bound: the farthest pair (query box, tile box) of the best tile holding >= K keys
  float ubw = INFINITY;
  for (int t = tid; t < ntiles; t += 64 * PW) {
    const float4 b0 = reinterpret_cast<const float4*>(box)[t * 2], b1 = reinterpret_cast<const float4*>(box)[t * 2 + 1];
    if (b1.z >= (float)K) {
      const float dx = fmaxf(b0.w - ql[0], qh[0] - b0.x), dy = fmaxf(b1.x - ql[1], qh[1] - b0.y),
                  dz = fmaxf(b1.y - ql[2], qh[2] - b0.z);
      ubw = fminf(ubw, (dx * dx + dy * dy + dz * dz) * 1.0001f + 1e-30f);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ubw = fminf(ubw, __shfl_xor(ubw, off));
  if (lane == 0) sub[wv][0] = ubw;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < PW; ++w) ubw = fminf(ubw, sub[w][0]);
  __syncthreads();

  double bd[K];
  int bi[K];
#pragma unroll
  for (int c = 0; c < K; ++c) {
    bd[c] = INFINITY;
    bi[c] = INT_MAX;
  }
  float ub = INFINITY;
  // Sweep 0 tightens the per-query bound over the candidate tiles, sweep 1 scans them. Tiles are taken
  // PCH at a time so that the candidate list always fits in LDS; with one chunk (the usual case) the
  // list of sweep 0 is reused.
  const bool one_chunk = ntiles <= PCH;
  for (int sweep = 0; sweep < 2; ++sweep) {
    for (int c0 = 0; c0 < ntiles; c0 += PCH) {
      if (sweep == 0 || !one_chunk) {
        // B. candidates of this chunk: tile boxes within ubw of the query box
        __syncthreads();
        if (tid == 0) ncand = 0;
        __syncthreads();
        for (int t = c0 + tid; t < min(ntiles, c0 + PCH); t += 64 * PW) {
          const float4 b0 = reinterpret_cast<const float4*>(box)[t * 2], b1 = reinterpret_cast<const float4*>(box)[t * 2 + 1];
          const float dx = fmaxf(fmaxf(b0.x - qh[0], ql[0] - b0.w), 0.f);
          const float dy = fmaxf(fmaxf(b0.y - qh[1], ql[1] - b1.x), 0.f);
          const float dz = fmaxf(fmaxf(b0.z - qh[2], ql[2] - b1.y), 0.f);
          if ((dx * dx + dy * dy + dz * dz) * 0.9999f <= ubw) {
            const int s = atomicAdd(&ncand, 1);
            cand[s] = t;
            cbox[s][0] = b0;
            cbox[s][1] = b1;
          }
        }
        __syncthreads();
      }
      const int nc = ncand;
      if (sweep == 0) {
        for (int c = wv; c < nc; c += PW) {
          const float4 b0 = cbox[c][0], b1 = cbox[c][1];
          if (b1.z >= (float)K) {
            const float dx = fmaxf(fabsf(fx - b0.x), fabsf(b0.w - fx));
            const float dy = fmaxf(fabsf(fy - b0.y), fabsf(b1.x - fy));
            const float dz = fmaxf(fabsf(fz - b0.z), fabsf(b1.y - fz));
            ub = fminf(ub, (dx * dx + dy * dy + dz * dz) * 1.0001f + 1e-30f);
          }
        }
        continue;
      }
      for (int c = wv; c < nc; c += PW) {
        const float4 b0 = cbox[c][0], b1 = cbox[c][1];
        const float dx = fmaxf(fmaxf(b0.x - fx, fx - b0.w), 0.f);
        const float dy = fmaxf(fmaxf(b0.y - fy, fy - b1.x), 0.f);
        const float dz = fmaxf(fmaxf(b0.z - fz, fz - b1.y), 0.f);
        const float mind = (dx * dx + dy * dy + dz * dz) * 0.9999f;
        const float thr = fminf(ub, (float)bd[K - 1] * 1.0001f);      // (float)inf stays inf
        if (!__any(mind <= thr)) continue;
        const int cntk = (int)b1.z;
        const int p = cand[c] * PT + lane;
        const bool has = lane < cntk;                                 // padding keys can never be inserted
        sk[wv][0][lane] = has ? skey[(int64_t)p * 3] : INFINITY;
        sk[wv][1][lane] = has ? skey[(int64_t)p * 3 + 1] : INFINITY;
        sk[wv][2][lane] = has ? skey[(int64_t)p * 3 + 2] : INFINITY;
        si[wv][lane] = has ? sidx[p] : INT_MAX;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        constexpr int U = 8;                                          // independent distance chains in flight
        for (int j0 = 0; j0 < PT; j0 += U) {
          double d2[U];
          int id[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            d2[u] = knn_d2(qx, qy, qz, sk[wv][0][j0 + u], sk[wv][1][j0 + u], sk[wv][2][j0 + u]);
            id[u] = si[wv][j0 + u];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) topk_insert<K, int>(bd, bi, d2[u], id[u]);
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (sweep == 0) {   // combine the per-wave partial bounds
      sub[wv][lane] = ub;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < PW; ++w) ub = fminf(ub, sub[w][lane]);
      if (!live) ub = -1.f;   // idle lanes never ask for a tile
    }
  }
  __syncthreads();   // the candidate list is dead: its bytes become the merge buffers
#pragma unroll
  for (int c = 0; c < K; ++c) {
    md[wv][lane][c] = bd[c];
    mi[wv][lane][c] = bi[c];
  }
  __syncthreads();
  if (wv == 0 && live) {
    for (int w = 1; w < PW; ++w)
#pragma unroll
      for (int c = 0; c < K; ++c) {
        const int id = mi[w][lane][c];
        if (id != INT_MAX) topk_insert<K, int>(bd, bi, md[w][lane][c], id);
      }
#pragma unroll
    for (int c = 0; c < K; ++c)
      if (c < kout) out[qi * kout + c] = bi[c] == INT_MAX ? -1 : (int64_t)bi[c];
  }
}
