// Greedy maximum coverage of one chunk by one workgroup, shared by csrc/scene_inputs.hip (select_frames_k: every chunk
// of ONE scene) and csrc/train_inputs.hip (train_select_frames_k: every item reads ITS scene's bit rows), so that both
// make the same choice by the same integer arithmetic:
//   step 1  the chunk's base points as a bit mask in LDS: a binary search of add + base_point_ind[b] in the chunk's
//           ascending row, 64 base points per ballot
//   step 2  nv rounds of popcount(row_f & alive) summed per wave, the first maximum, alive &= ~row_pick
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int SF_T = 512;        // threads of a selection workgroup: 8 waves share out the frames
constexpr int SF_WAVES = SF_T / 64;

// is v among row[0 .. n) (ascending, distinct)?
__device__ __forceinline__ bool row_holds(const int64_t* __restrict__ row, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (row[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < n && row[lo] == v;
}

// the better of two (count, frame) pairs: the larger count, the lower frame among equals
__device__ __forceinline__ void take_better(int& c, int& f, int oc, int of) {
  if (oc > c || (oc == c && of < f)) {
    c = oc;
    f = of;
  }
}

// All SF_T threads of the workgroup call it with the same arguments. packed: the scene's [nf][W] bit rows;
// base_point_ind [nb]; the chunk is row[0 .. n), and base point b belongs to it when add + base_point_ind[b] is found
// there. s_alive: W words and s_count: nf ints of LDS, s_pick: one int of LDS. sel_out [nv].
__device__ __forceinline__ void select_frames_wg(const uint32_t* __restrict__ packed, int nb, int nf, int W,
                                                 const int64_t* __restrict__ base_point_ind, int64_t add,
                                                 const int64_t* __restrict__ row, int64_t n, int nv,
                                                 int32_t* __restrict__ sel_out, uint32_t* s_alive, int* s_count,
                                                 int* s_pick) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // step 1: 64 base points per ballot are two words of the mask
  for (int b0 = wave * 64; b0 < nb; b0 += SF_T) {
    const int b = b0 + lane;
    const bool in = b < nb && n > 0 && row_holds(row, n, add + base_point_ind[b]);
    const unsigned long long m = __ballot(in);
    if (lane == 0) {
      const int w = b0 >> 5;
      s_alive[w] = (uint32_t)m;
      if (w + 1 < W) s_alive[w + 1] = (uint32_t)(m >> 32);
    }
  }
  __syncthreads();

  // step 2
  for (int r = 0; r < nv; ++r) {
    for (int f = wave; f < nf; f += SF_WAVES) {
      const uint32_t* __restrict__ bits = packed + (int64_t)f * W;
      int c = 0;
      for (int w = lane; w < W; w += 64) c += __popc(bits[w] & s_alive[w]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
      if (lane == 0) s_count[f] = c;
    }
    __syncthreads();
    if (wave == 0) {
      int bc = -1, bf = nf;
      for (int f = lane; f < nf; f += 64) take_better(bc, bf, s_count[f], f);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(bc, o), of = __shfl_xor(bf, o);
        take_better(bc, bf, oc, of);
      }
      if (lane == 0) {
        *s_pick = bf;
        sel_out[r] = bf;
      }
    }
    __syncthreads();
    const uint32_t* __restrict__ bits = packed + (int64_t)(*s_pick) * W;
    for (int w = threadIdx.x; w < W; w += SF_T) s_alive[w] &= ~bits[w];
    __syncthreads();
  }
}
