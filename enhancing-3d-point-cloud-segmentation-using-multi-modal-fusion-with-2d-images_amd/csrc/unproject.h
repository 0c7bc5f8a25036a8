// Depth back-projection of one pixel, shared by csrc/fusion.hip (unproject_kernel) and csrc/scene_inputs.hip
// (chunk_unproject_k) so that both evaluate the same float64 expression in the same order (both files are compiled with
// -ffp-contract=off):  xyz_cam = (Kinv . [u, v, 1]) * depth ;  xyz_world = xyz_cam . R^T + t
#pragma once
#include <stdint.h>

struct Cam {
  double kinv[9];
};

// c: camera coordinates (c[2] > 0 is the pixel's validity), x: world coordinates. P: the view's 4 x 4 float32 pose.
__device__ __forceinline__ void unproject_pixel(const Cam& cam, const float* __restrict__ P, double u, double v,
                                                uint16_t depth_mm, double (&c)[3], double (&x)[3]) {
  // depth: uint16 mm -> float32 / 1000.f (ScanNet_sphere_color.py:410), then promoted to float64
  const double d = (double)((float)depth_mm / 1000.f);
#pragma unroll
  for (int r = 0; r < 3; ++r) c[r] = ((cam.kinv[r * 3] * u + cam.kinv[r * 3 + 1] * v) + cam.kinv[r * 3 + 2]) * d;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    x[r] = ((c[0] * (double)P[r * 4] + c[1] * (double)P[r * 4 + 1]) + c[2] * (double)P[r * 4 + 2]) + (double)P[r * 4 + 3];
}
