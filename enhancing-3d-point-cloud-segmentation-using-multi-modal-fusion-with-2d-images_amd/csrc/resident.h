// The resident scenes of include/mvkpconv_train.h (points, base points, bit rows and frames of S scenes one after
// another, described by scenes [S,8] int64), shared by csrc/train_inputs.hip and csrc/sphere_inputs.hip so that both
// check an item's row against the totals by the same rule: a row that leaves them is an empty scene.
#pragma once
#include "common.h"

constexpr int64_t MAX_SIZE = (int64_t)1 << 31;

struct Totals {
  int64_t P, NB, F, NW;
};

struct Scene {
  int64_t point_off, num_points, base_off, num_base, frame_off, num_frames, bits_off;
  bool ok;
};

// Row `id` of the table, checked against the totals: a row that leaves them is an empty scene.
__device__ __forceinline__ Scene load_scene(const int64_t* __restrict__ scenes, int S, const Totals& t, int64_t id) {
  Scene s = {0, 0, 0, 0, 0, 0, 0, false};
  if (id < 0 || id >= S) return s;
  const int64_t* __restrict__ r = scenes + id * 8;
  const int64_t po = r[0], np = r[1], bo = r[2], nb = r[3], fo = r[4], nf = r[5], wo = r[6];
  if (po < 0 || np < 0 || po > t.P || np > t.P - po || bo < 0 || nb < 0 || bo > t.NB || nb > t.NB - bo || fo < 0 ||
      nf < 0 || fo > t.F || nf > t.F - fo || wo < 0 || wo > t.NW || nf * ((nb + 31) >> 5) > t.NW - wo)
    return s;
  s = {po, np, bo, nb, fo, nf, wo, true};
  return s;
}

static inline bool totals_ok(int64_t P, int64_t NB, int64_t F, int64_t NW, int S) {
  return P >= 0 && NB >= 0 && F >= 0 && NW >= 0 && S >= 0 && P < MAX_SIZE && NB < MAX_SIZE && F < MAX_SIZE && NW < MAX_SIZE;
}

