// The strided map that the row kernels (pn2_rows.hip) read and scatter onto and that the ordered walk (pn2_ordered.hip)
// stores through, and the size refusals of the entries on either side.
#pragma once
#include "common.h"

constexpr int64_t ROWS_LIMIT = (int64_t)1 << 31;

// element (image i, channel c, pixel q) at i * si + c * sc + q * sp. A 2D encoder's map is NCHW (C*hw, hw, 1) or
// channels-last (C*hw, 1, C); a point feature (B, C, N) is one image of N pixels per batch element: (C*N, N, 1).
struct MapStrides {
  int64_t si, sc, sp;
};

// the offset of channel 0 of key p in [0, nv*hw) of batch element b (nv images of hw pixels each). Every entry refuses
// nv*hw >= 2^31, so the image of a key is a 32-bit division; one image needs none.
__device__ __forceinline__ int64_t map_offset(int64_t p, int64_t b, int64_t nv, int64_t hw, MapStrides s) {
  const int64_t view = nv == 1 ? 0 : (int64_t)((uint32_t)p / (uint32_t)hw);
  return (b * nv + view) * s.si + (p - view * hw) * s.sp;
}

// the same for an index as a caller gave it: -1 for a key outside [0, nv*hw)
__device__ __forceinline__ int64_t map_pixel(int64_t p, int64_t b, int64_t nv, int64_t hw, MapStrides s) {
  return p < 0 || p >= nv * hw ? -1 : map_offset(p, b, nv, hw, s);
}

// SetAbstraction: R = B*M*K rows over B*N points
inline int rows_sizes(const char* what, int B, int C, int64_t N, int64_t M, int K, int64_t* R) {
  MVK_REQUIRE(B >= 0 && C >= 0 && N >= 0 && M >= 0 && K >= 0, "%s: bad sizes B=%d C=%d N=%lld M=%lld K=%d", what, B, C,
              (long long)N, (long long)M, K);
  MVK_REQUIRE(M == 0 || K == 0 || ((int64_t)B * M < ROWS_LIMIT && (int64_t)B * M * K < ROWS_LIMIT),
              "%s: R = B*M*K = %d*%lld*%d must be below 2^31", what, B, (long long)M, K);
  MVK_REQUIRE((int64_t)B * N < ROWS_LIMIT, "%s: B*N must be below 2^31", what);
  *R = (int64_t)B * M * K;
  return 0;
}

// FeatureAggregation: R = B*np*K rows over B*nv*hw pixels
inline int fa_sizes(const char* what, int B, int nv, int C, int64_t hw, int64_t np, int K, MapStrides s, int64_t* R,
                    int64_t* P) {
  MVK_REQUIRE(B >= 0 && nv >= 0 && C >= 0 && hw >= 0 && np >= 0 && K >= 0,
              "%s: bad sizes B=%d nv=%d C=%d hw=%lld np=%lld k=%d", what, B, nv, C, (long long)hw, (long long)np, K);
  MVK_REQUIRE(s.si >= 0 && s.sc >= 0 && s.sp >= 0, "%s: negative map stride", what);
  MVK_REQUIRE(np == 0 || K == 0 || ((int64_t)B * np < ROWS_LIMIT && (int64_t)B * np * K < ROWS_LIMIT),
              "%s: R = B*np*k = %d*%lld*%d must be below 2^31", what, B, (long long)np, K);
  MVK_REQUIRE(hw < ROWS_LIMIT && (int64_t)nv * hw < ROWS_LIMIT && (int64_t)B * nv * hw < ROWS_LIMIT,
              "%s: B*nv*hw = %d*%d*%lld must be below 2^31", what, B, nv, (long long)hw);
  *R = (int64_t)B * np * K;
  *P = (int64_t)nv * hw;
  return 0;
}
