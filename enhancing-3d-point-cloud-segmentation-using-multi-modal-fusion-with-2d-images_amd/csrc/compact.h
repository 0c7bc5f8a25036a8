// Ordered stream compaction in 1024-point blocks, shared by the sphere query (fusion.hip) and the chunk boxes
// (chunk.hip): per-block ballot counts -> exclusive scan of the block counts -> scatter at block offset + rank, so the
// members come out in ascending index order.
#pragma once
#include <hip/hip_runtime.h>

constexpr int COMPACT_T = 1024;               // points (threads) per block
constexpr int COMPACT_WAVES = COMPACT_T / 64;

// rank of a member lane among the members of its wave (m = the wave's ballot)
__device__ __forceinline__ int compact_lane_rank(unsigned long long m) {
  return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// members in the waves in front of wave w of this block (wave_counts: the block's per-wave popcounts)
__device__ __forceinline__ int compact_wave_offset(const int* wave_counts, int w) {
  int off = 0;
  for (int k = 0; k < w; ++k) off += wave_counts[k];
  return off;
}

// One workgroup of COMPACT_T threads: exclusive scan of block_count[0..nblk) in place; returns the total to every
// thread. carry / ws: one int and COMPACT_WAVES ints of LDS.
__device__ __forceinline__ int compact_scan_counts(int* __restrict__ block_count, int nblk, int* carry, int* ws) {
  if (threadIdx.x == 0) *carry = 0;
  __syncthreads();
  for (int base = 0; base < nblk; base += COMPACT_T) {
    const int i = base + threadIdx.x;
    const int v = i < nblk ? block_count[i] : 0;
    int x = v;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) ws[w] = x;
    __syncthreads();
    int off = *carry;
    for (int k = 0; k < w; ++k) off += ws[k];
    if (i < nblk) block_count[i] = off + x - v;
    __syncthreads();
    if (threadIdx.x == COMPACT_T - 1) *carry = off + x;
    __syncthreads();
  }
  return *carry;
}
