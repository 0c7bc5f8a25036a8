// Membership of a sphere around a float64 centre and the Tukey weight of the sampling potentials, shared by the
// one-sphere entry points (mvk_ball_query / mvk_tukey_update, csrc/fusion.hip) and the batched ones
// (csrc/sphere_inputs.hip) so that the two cannot differ. Include from a translation unit compiled with -ffp-contract=off.
#pragma once
#include "common.h"

struct Ball {
  double cx, cy, cz, r2;
};

// sklearn's euclidean rdist on the float32 point promoted to float64: dx^2 + dy^2 + dz^2, summed in this order
__device__ __forceinline__ double ball_rdist(const float* __restrict__ pts, int64_t i, const Ball& b) {
  const double dx = (double)pts[i * 3] - b.cx, dy = (double)pts[i * 3 + 1] - b.cy, dz = (double)pts[i * 3 + 2] - b.cz;
  double d2 = 0.0;
  d2 += dx * dx;
  d2 += dy * dy;
  d2 += dz * dz;
  return d2;
}

// what a member at rdist rd <= r2 adds to its potential (ScanNet_sphere_color.py:575-579)
__device__ __forceinline__ double tukey_weight(double rd, double r2) {
  const double d = sqrt(rd);          // query_radius returns dist = sqrt(rdist) ...
  const double d2s = d * d;           // ... and the reference squares it again (:575)
  double t = 1.0 - d2s / r2;
  t = t * t;
  if (d2s > r2) t = 0.0;              // :579
  return t;
}
