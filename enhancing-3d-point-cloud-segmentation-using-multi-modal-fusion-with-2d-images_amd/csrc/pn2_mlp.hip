// Frozen PointNet++ inference: a SetAbstraction's "group, concatenate, shared MLP, max over the neighbours"
// and a FeaturePropagation's "interpolate, concatenate, shared MLP" as one launch each. The grouped (B,C,M,K) tensor and
// the activations between the layers never leave the workgroup: a tile of R rows (neighbours of some centroids, or dense
// points) is staged into LDS, up to three layers y = relu(W x + b) run on it with v_mfma_f32_16x16x4_f32 (exact f32, a
// k-ordered fma chain per output), ping-ponging between two LDS buffers, and only the result goes to HBM. A third front
// end on the same core is MVPNet3D's FeatureAggregation fed from the 2D encoder's map: gather by flat pixel
// index, relation channels, shared MLP, sum or max over the neighbours.
//
// Contraction: this file is compiled with -ffp-contract=off (build.py), like pn2.hip. The layers lose nothing by it: their
// products are MFMA builtins, which the flag does not touch, and the staging is loads and one subtraction. The one piece
// that must reproduce another kernel bit for bit, the 3-NN interpolation (mvk_interpolate_fwd of pn2.hip: a rounded
// product, then a rounded sum), needs it: it is written with __fmul_rn / __fadd_rn to say so, but in the HIP headers
// those are a plain product and sum, which the default (contraction on) fuses into an fma -- measured on the device as
// last-bit differences from feature_interpolate before the flag was set.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MT = 256;                 // 4 waves
constexpr int MAXL = 3;
constexpr int MAX_IN = 768;             // widest input row (FeaturePropagation level 0 of PN2SSG: 512 + 256)
constexpr int MAX_W = 512;              // widest layer
constexpr int LDS_LIMIT = 160 * 1024;   // per workgroup on gfx950
constexpr int LDS_TARGET = 64 * 1024;   // larger tiles are only chosen below this (two or more workgroups per CU)

struct Chain {
  int n_layers;
  int width[MAXL + 1];
  int w_off[MAXL], b_off[MAXL];         // float offsets of W_l [width[l+1], width[l]] and b_l in the packed buffer
  int vec[MAXL];                        // rows of W_l can be read as aligned float4
  int stride[2];                        // LDS row strides (floats) of the two activation buffers
  int relu_last;
};

__host__ __device__ inline int pad16(int c) { return (c + 15) & ~15; }

// One layer on a tile of R rows (R a multiple of 32): out[r][n] = act(b[n] + sum_k W[n][k] in[r][k]) for n < pad16(Cout);
// columns in [Cout, pad16(Cout)) come out as 0, which is what the next layer's k loop expects of its input (`in` must
// have zeros in [Cin, pad16(Cin)) too). A wave owns units of 16 channels x 32 rows: W is the A operand (lane l supplies
// W[n0 + (l & 15)][k0 + 4 (l >> 4) + j] to the j-th of four MFMAs, one float4 from L2 per 16 k), the rows are the B operand
// (the same float4 pattern from LDS), so D holds four consecutive channels of one row per lane: one 16-byte LDS store.
__device__ __forceinline__ void mlp_layer(const float* __restrict__ W, const float* __restrict__ bias, int Cin, int Cout,
                                          bool vec, bool relu, const float* in, int si, float* out, int so, int R) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int nct = pad16(Cout) >> 4, units = nct * (R >> 5);
  const int kend = pad16(Cin);
  for (int u = wave; u < units; u += MT / 64) {
    const int ct = u % nct, pg = u / nct;
    const int n = ct * 16 + r16;
    const bool n_ok = n < Cout;
    const float* wrow = W + (int64_t)(n_ok ? n : 0) * Cin;
    const float* x0 = in + (pg * 32 + r16) * si + 4 * q;
    const float* x1 = x0 + 16 * si;
    f32x4 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = ct * 16 + 4 * q + i;
      const float bv = c < Cout ? bias[c] : 0.0f;
      acc0[i] = bv;
      acc1[i] = bv;
    }
    auto load_w = [&](int k0) {
      const int k = k0 + 4 * q;
      f32x4 w = {0.0f, 0.0f, 0.0f, 0.0f};
      if (vec) {
        if (n_ok && k < Cin) w = *reinterpret_cast<const f32x4*>(wrow + k);
      } else if (n_ok) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < Cin) w[j] = wrow[k + j];
      }
      return w;
    };
    f32x4 w = load_w(0);
    for (int k0 = 0; k0 < kend; k0 += 16) {
      f32x4 wn = {0.0f, 0.0f, 0.0f, 0.0f};
      if (k0 + 16 < kend) wn = load_w(k0 + 16);      // one step ahead of the MFMAs that hide its latency
      const f32x4 a = *reinterpret_cast<const f32x4*>(x0 + k0);
      const f32x4 b = *reinterpret_cast<const f32x4*>(x1 + k0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j], a[j], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j], b[j], acc1, 0, 0, 0);
      }
      w = wn;
    }
    if (relu) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc0[i] = fmaxf(acc0[i], 0.0f);
        acc1[i] = fmaxf(acc1[i], 0.0f);
      }
    }
    float* o = out + (pg * 32 + r16) * so + ct * 16 + 4 * q;
    *reinterpret_cast<f32x4*>(o) = acc0;
    *reinterpret_cast<f32x4*>(o + 16 * so) = acc1;
  }
}

// The whole chain on the tile staged in buf0; returns the buffer that holds the last layer's output. Ends on a barrier.
__device__ __forceinline__ const float* mlp_chain(const Chain& ch, const float* __restrict__ params, float* buf0,
                                                  float* buf1, int R, int* stride_out) {
  float* cur = buf0;
  float* nxt = buf1;
  int sc = ch.stride[0], sn = ch.stride[1];
  for (int l = 0; l < ch.n_layers; ++l) {
    mlp_layer(params + ch.w_off[l], params + ch.b_off[l], ch.width[l], ch.width[l + 1], ch.vec[l] != 0,
              ch.relu_last || l + 1 < ch.n_layers, cur, sc, nxt, sn, R);
    __syncthreads();
    float* t = cur; cur = nxt; nxt = t;
    const int ts = sc; sc = sn; sn = ts;
  }
  *stride_out = sc;
  return cur;
}

// Set abstraction. Grid (ceil(M / G), B). G > 1: the tile holds all K neighbours of G centroids (G K <= R), one pass.
// G == 1: one centroid per workgroup, its K rows in passes of R, a running maximum per channel in registers.
__global__ __launch_bounds__(MT) void pn2_sa_k(const float* __restrict__ xyz, const float* __restrict__ feature,
                                               const float* __restrict__ new_xyz, const int64_t* __restrict__ index,
                                               const float* __restrict__ params, Chain ch, int C, int has_xyz, int64_t N,
                                               int64_t M, int K, int rshift, int G, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int R = 1 << rshift, t = threadIdx.x;
  float* buf0 = lds;
  float* buf1 = buf0 + R * ch.stride[0];
  int* ridx = reinterpret_cast<int*>(buf1 + R * ch.stride[1]);       // key of the row: >= 0, -1 outside [0, N), -2 no row
  int* rcen = ridx + R;                                              // centroid of the row, relative to m0
  const int64_t b = blockIdx.y, m0 = (int64_t)blockIdx.x * G;
  const int gcnt = (int)(M - m0 < G ? M - m0 : G);
  const int Cin = ch.width[0], kpad = pad16(Cin), Cout = ch.width[ch.n_layers];
  const int passes = G > 1 ? 1 : (K + R - 1) / R;
  float run[2] = {-INFINITY, -INFINITY};
  for (int pass = 0; pass < passes; ++pass) {
    const int kbase = pass * R;
    const int rows = G > 1 ? gcnt * K : (K - kbase < R ? K - kbase : R);
    for (int r = t; r < R; r += MT) {
      int v = -2, g = 0;
      if (r < rows) {
        g = G > 1 ? r / K : 0;
        const int k = G > 1 ? r - g * K : kbase + r;
        const int64_t j = index[((b * M + m0 + g) * K) + k];
        v = (j >= 0 && j < N) ? (int)j : -1;
      }
      ridx[r] = v;
      rcen[r] = g;
    }
    __syncthreads();
    // [feature(idx) | xyz(idx) - new_xyz], lanes along the rows; an index outside [0, N) reads as zero BEFORE the subtraction
    for (int e = t; e < (kpad << rshift); e += MT) {
      const int r = e & (R - 1), c = e >> rshift;
      const int j = ridx[r];
      float v = 0.0f;
      if (j != -2 && c < Cin) {
        if (c < C) {
          v = j >= 0 ? feature[(b * C + c) * N + j] : 0.0f;
        } else if (has_xyz) {
          const int d = c - C;
          v = (j >= 0 ? xyz[(b * 3 + d) * N + j] : 0.0f) - new_xyz[(b * 3 + d) * M + m0 + rcen[r]];
        }
      }
      buf0[r * ch.stride[0] + c] = v;
    }
    __syncthreads();
    int sf;
    const float* y = mlp_chain(ch, params, buf0, buf1, R, &sf);
    if (G > 1) {
      for (int e = t; e < gcnt * Cout; e += MT) {
        const int g = e % gcnt, c = e / gcnt;
        const float* col = y + g * K * sf + c;
        float mx = col[0];
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, col[k * sf]);
        out[(b * Cout + c) * M + m0 + g] = mx;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = t + i * MT;
        if (c < Cout)
          for (int r = 0; r < rows; ++r) run[i] = fmaxf(run[i], y[r * sf + c]);
      }
      __syncthreads();            // the next pass stages over these buffers
    }
  }
  if (G == 1) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = t + i * MT;
      if (c < Cout) out[(b * Cout + c) * M + m0] = run[i];
    }
  }
}

// Propagation / head. Grid (ceil(N1 / R), B); rows are dense points. index == NULL: the row is dense_feature alone.
__global__ __launch_bounds__(MT) void pn2_fp_k(const float* __restrict__ sparse, const int64_t* __restrict__ index,
                                               const float* __restrict__ weight, const float* __restrict__ dense,
                                               const float* __restrict__ params, Chain ch, int C2, int C1, int64_t N2,
                                               int64_t N1, int rshift, float* __restrict__ out,
                                               int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int R = 1 << rshift, t = threadIdx.x;
  float* buf0 = lds;
  float* buf1 = buf0 + R * ch.stride[0];
  int* rix = reinterpret_cast<int*>(buf1 + R * ch.stride[1]);        // [R][3] keys, -1 outside [0, N2)
  float* rw = reinterpret_cast<float*>(rix + 3 * R);                 // [R][3] weights
  const int64_t b = blockIdx.y, n0 = (int64_t)blockIdx.x << rshift;
  const int rows = (int)(N1 - n0 < R ? N1 - n0 : R);
  const int Cin = ch.width[0], kpad = pad16(Cin), Cout = ch.width[ch.n_layers];
  if (C2 > 0) {
    bool bad = false;
    for (int e = t; e < 3 * rows; e += MT) {
      const int64_t j = index[(b * N1 + n0) * 3 + e];
      const bool ok = j >= 0 && j < N2;
      rix[e] = ok ? (int)j : -1;
      rw[e] = weight[(b * N1 + n0) * 3 + e];
      bad |= !ok;
    }
    if (bad && status) *status = 1;
    __syncthreads();
  }
  // [interpolated (C2) | dense (C1)], lanes along the rows
  for (int e = t; e < (kpad << rshift); e += MT) {
    const int r = e & (R - 1), c = e >> rshift;
    float v = 0.0f;
    if (r < rows && c < Cin) {
      if (c < C2) {
        const float* f = sparse + (b * C2 + c) * N2;
        // mvk_interpolate_fwd bit for bit: k = 0, 1, 2 in order, a rounded product and a rounded sum each
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int j = rix[3 * r + k];
          if (j >= 0) v = __fadd_rn(v, __fmul_rn(f[j], rw[3 * r + k]));
        }
      } else {
        v = dense[(b * C1 + (c - C2)) * N1 + n0 + r];
      }
    }
    buf0[r * ch.stride[0] + c] = v;
  }
  __syncthreads();
  int sf;
  const float* y = mlp_chain(ch, params, buf0, buf1, R, &sf);
  for (int e = t; e < (Cout << rshift); e += MT) {
    const int r = e & (R - 1), c = e >> rshift;
    if (r < rows) out[(b * Cout + c) * N1 + n0 + r] = y[r * sf + c];
  }
}

// Feature aggregation. Grid (ceil(N / G), B); the tile holds all K rows of G = R / K points, one pass. Row
// (n, k) with j = index[b, n, k]: [feat(image j / HW, c, pixel j % HW) for c < C | diff_0..2 | dist], diff_d =
// image_xyz[b, j, d] - points[b, d, n], dist = (diff_0^2 + diff_1^2) + diff_2^2; j outside [0, P) reads as zero for the
// features and for image_xyz BEFORE the subtraction. feat is addressed through element strides (image, channel,
// pixel): an NCHW map puts lanes along the rows (each lane's read stays in one channel plane, like group_points), a
// channels-last map (sc == 1) puts 16 lanes along the channels of one row. The reduction over k (sum in ascending k
// from the k = 0 value, or fmaxf) reads the last layer's outputs from LDS with lanes along the points. Cloud b is its
// first nb = clamp(lengths[b], 1, N) columns: the columns behind are stored as zeros and their indices never read.
__global__ __launch_bounds__(MT) void pn2_fa_k(const float* __restrict__ feat, int64_t si, int64_t sc, int64_t sp,
                                               const float* __restrict__ image_xyz, const float* __restrict__ points,
                                               const int64_t* __restrict__ index, const int64_t* __restrict__ lengths,
                                               const float* __restrict__ params, Chain ch, int C, int nv, int HW, int64_t N,
                                               int K, int rshift, int G, int reduce, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int R = 1 << rshift, t = threadIdx.x;
  float* buf0 = lds;
  float* buf1 = buf0 + R * ch.stride[0];
  int64_t* roff = reinterpret_cast<int64_t*>(buf1 + R * ch.stride[1]);   // image * si + pixel * sp of the row's pixel
  int* ridx = reinterpret_cast<int*>(roff + R);                          // key of the row: >= 0, -1 outside [0, P), -2 no row
  int* rcen = ridx + R;                                                  // point of the row, relative to n0
  const int64_t b = blockIdx.y, n0 = (int64_t)blockIdx.x * G, P = (int64_t)nv * HW;
  int64_t nb = N;
  if (lengths) {
    nb = lengths[b];
    nb = nb < 1 ? 1 : (nb > N ? N : nb);
  }
  const int cols = (int)(N - n0 < G ? N - n0 : G);                       // columns of `out` this workgroup owns
  const int gcnt = nb - n0 >= cols ? cols : (nb > n0 ? (int)(nb - n0) : 0);   // of which valid
  const int Cin = ch.width[0], kpad = pad16(Cin), Cout = ch.width[ch.n_layers];
  for (int e = t; e < (cols - gcnt) * Cout; e += MT) {
    const int g = gcnt + e % (cols - gcnt), c = e / (cols - gcnt);
    out[(b * Cout + c) * N + n0 + g] = 0.0f;
  }
  if (gcnt == 0) return;
  const int rows = gcnt * K;
  for (int r = t; r < R; r += MT) {
    int v = -2, g = 0;
    int64_t off = 0;
    if (r < rows) {
      g = r / K;
      const int64_t j = index[(b * N + n0 + g) * K + (r - g * K)];
      v = -1;
      if (j >= 0 && j < P) {
        v = (int)j;
        const int img = v / HW;
        off = img * si + (v - img * HW) * sp;
      }
    }
    roff[r] = off;
    ridx[r] = v;
    rcen[r] = g;
  }
  __syncthreads();
  const float* fb = feat + b * nv * si;
  const float* xb = image_xyz + b * P * 3;
  const float* pb = points + b * 3 * N + n0;
  const bool along_c = sc == 1 && C > 1;
  for (int e = t; e < (kpad << rshift); e += MT) {
    const int r = along_c ? (e >> 4) & (R - 1) : e & (R - 1);
    const int c = along_c ? (e & 15) + ((e >> (4 + rshift)) << 4) : e >> rshift;
    const int j = ridx[r];
    float v = 0.0f;
    if (j != -2 && c < Cin) {
      if (c < C) {
        v = j >= 0 ? fb[roff[r] + c * sc] : 0.0f;
      } else {
        const int d = c - C, g = rcen[r];
        if (d < 3) {
          v = (j >= 0 ? xb[(int64_t)j * 3 + d] : 0.0f) - pb[d * N + g];
        } else {
          const float d0 = (j >= 0 ? xb[(int64_t)j * 3] : 0.0f) - pb[g];
          const float d1 = (j >= 0 ? xb[(int64_t)j * 3 + 1] : 0.0f) - pb[N + g];
          const float d2 = (j >= 0 ? xb[(int64_t)j * 3 + 2] : 0.0f) - pb[2 * N + g];
          v = (d0 * d0 + d1 * d1) + d2 * d2;
        }
      }
    }
    buf0[r * ch.stride[0] + c] = v;
  }
  __syncthreads();
  int sf;
  const float* y = mlp_chain(ch, params, buf0, buf1, R, &sf);
  for (int e = t; e < gcnt * Cout; e += MT) {
    const int g = e % gcnt, c = e / gcnt;
    const float* col = y + g * K * sf + c;
    float acc = col[0];
    if (reduce) {
      for (int k = 1; k < K; ++k) acc = fmaxf(acc, col[k * sf]);
    } else {
      for (int k = 1; k < K; ++k) acc = acc + col[k * sf];
    }
    out[(b * Cout + c) * N + n0 + g] = acc;
  }
}

// Bytes of LDS of a tile of R rows: the two activation buffers and `aux` words per row of the front end's own.
inline int64_t lds_bytes(const Chain& ch, int R, int aux) {
  return (int64_t)R * (ch.stride[0] + ch.stride[1] + aux) * 4;
}
constexpr int AUX_SA = 2, AUX_FP = 6, AUX_FA = 4, AUX_MAX = 6;

// Widths, offsets and LDS strides of a chain, and the one statement of what is supported. Returns 0, or -1 with the
// error set.
int make_chain(const char* who, const float* params, const int* widths_host, int n_layers, int relu_last, Chain* ch) {
  MVK_REQUIRE(n_layers >= 1 && n_layers <= MAXL, "%s: %d layers (1 .. %d are supported)", who, n_layers, MAXL);
  MVK_REQUIRE(widths_host, "%s: null widths", who);
  MVK_REQUIRE(widths_host[0] >= 1 && widths_host[0] <= MAX_IN, "%s: input rows of %d values (1 .. %d are supported)", who,
              widths_host[0], MAX_IN);
  ch->n_layers = n_layers;
  ch->relu_last = relu_last ? 1 : 0;
  int off = 0, s[2] = {0, 0};
  for (int l = 0; l <= n_layers; ++l) {
    const int w = widths_host[l];
    if (l > 0) MVK_REQUIRE(w >= 1 && w <= MAX_W, "%s: layer %d is %d wide (1 .. %d are supported)", who, l - 1, w, MAX_W);
    ch->width[l] = w;
    if (pad16(w) + 4 > s[l & 1]) s[l & 1] = pad16(w) + 4;
  }
  for (int l = n_layers + 1; l <= MAXL; ++l) ch->width[l] = 0;
  for (int l = 0; l < MAXL; ++l) {
    ch->w_off[l] = ch->b_off[l] = ch->vec[l] = 0;
    if (l >= n_layers) continue;
    ch->w_off[l] = off;
    ch->vec[l] = (ch->width[l] % 4 == 0) && (off % 4 == 0) && (((uintptr_t)params & 15) == 0);
    off += ch->width[l + 1] * ch->width[l];
    ch->b_off[l] = off;
    off += ch->width[l + 1];
  }
  ch->stride[0] = s[0];
  ch->stride[1] = s[1];
  MVK_REQUIRE(lds_bytes(*ch, 32, AUX_MAX) <= LDS_LIMIT, "%s: widths %d, %d, %d, %d need %lld bytes of LDS (limit %d)", who,
              ch->width[0], ch->width[1], ch->width[2], ch->width[3], (long long)lds_bytes(*ch, 32, AUX_MAX), LDS_LIMIT);
  return 0;
}

// Rows per tile: at least 32 and, while the LDS holds it, at least `at_least` (a centroid's K rows in one pass); then 64
// or 128 while the tile stays below LDS_TARGET and the grid keeps 512 workgroups.
int pick_rshift(const Chain& ch, int aux, int64_t total_rows, int at_least) {
  int rs = 5;
  while (rs < 7 && (1 << rs) < at_least && lds_bytes(ch, 2 << rs, aux) <= LDS_LIMIT) ++rs;
  while (rs < 7 && lds_bytes(ch, 2 << rs, aux) <= LDS_TARGET && total_rows / (2 << rs) >= 512) ++rs;
  return rs;
}

template <typename Kern>
int allow_lds(Kern k, int64_t lds) {
  if (lds > 64 * 1024)
    MVK_CHECK_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}

}  // namespace

extern "C" int mvk_pn2_mlp_supported(const int* widths_host, int n_layers) {
  Chain ch;
  return make_chain("pn2_mlp_supported", nullptr, widths_host, n_layers, 1, &ch) == 0 ? 1 : 0;
}

extern "C" int mvk_pn2_sa_fwd(const float* xyz, const float* feature, const float* new_xyz, const int64_t* index,
                              const float* params, const int* widths_host, int n_layers, int B, int C, int use_xyz,
                              int64_t N, int64_t M, int K, float* out, void* stream) {
  Chain ch;
  if (make_chain("pn2_sa_fwd", params, widths_host, n_layers, 1, &ch)) return -1;
  MVK_REQUIRE(K >= 1, "pn2_sa_fwd: K = %d neighbours (need K >= 1)", K);
  MVK_REQUIRE(B >= 0 && B < 65536 && C >= 0 && N >= 1 && N < ((int64_t)1 << 31) && M >= 0,
              "pn2_sa_fwd: bad sizes B=%d C=%d N=%lld M=%lld", B, C, (long long)N, (long long)M);
  if (!feature) C = 0;
  const int has_xyz = (C == 0 || use_xyz) ? 1 : 0;
  MVK_REQUIRE(ch.width[0] == C + 3 * has_xyz, "pn2_sa_fwd: widths[0] = %d, the input rows hold %d values", ch.width[0],
              C + 3 * has_xyz);
  if (B == 0 || M == 0) return 0;
  MVK_REQUIRE(xyz && new_xyz && index && params && out, "pn2_sa_fwd: null operand");
  const int rs = pick_rshift(ch, AUX_SA, (int64_t)B * M * K, K);
  const int R = 1 << rs, G = K <= R ? R / K : 1;
  const int64_t gx = cdiv64(M, G), lds = lds_bytes(ch, R, AUX_SA);
  MVK_REQUIRE(gx < ((int64_t)1 << 31), "pn2_sa_fwd: too many centroids");
  if (allow_lds(pn2_sa_k, lds)) return -2;
  hipLaunchKernelGGL(pn2_sa_k, dim3((unsigned)gx, (unsigned)B), dim3(MT), (size_t)lds, (hipStream_t)stream, xyz, feature,
                     new_xyz, index, params, ch, C, has_xyz, N, M, K, rs, G, out);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_fp_fwd(const float* sparse_feature, const int64_t* index, const float* weight,
                              const float* dense_feature, const float* params, const int* widths_host, int n_layers,
                              int relu_last, int B, int C2, int C1, int64_t N2, int64_t N1, float* out, int32_t* status,
                              void* stream) {
  Chain ch;
  if (make_chain("pn2_fp_fwd", params, widths_host, n_layers, relu_last, &ch)) return -1;
  MVK_REQUIRE(B >= 0 && B < 65536 && C2 >= 0 && C1 >= 0 && N1 >= 0 && N2 >= 0 && N2 < ((int64_t)1 << 31),
              "pn2_fp_fwd: bad sizes B=%d C2=%d C1=%d N2=%lld N1=%lld", B, C2, C1, (long long)N2, (long long)N1);
  if (!index) C2 = 0;
  if (!dense_feature) C1 = 0;
  MVK_REQUIRE(ch.width[0] == C2 + C1, "pn2_fp_fwd: widths[0] = %d, the input rows hold %d + %d values", ch.width[0], C2, C1);
  if (B == 0 || N1 == 0) return 0;
  MVK_REQUIRE(params && out && (C2 == 0 || (sparse_feature && weight)), "pn2_fp_fwd: null operand");
  const int rs = pick_rshift(ch, AUX_FP, (int64_t)B * N1, 1);
  const int64_t gx = cdiv64(N1, (int64_t)1 << rs), lds = lds_bytes(ch, 1 << rs, AUX_FP);
  MVK_REQUIRE(gx < ((int64_t)1 << 31), "pn2_fp_fwd: too many points");
  if (allow_lds(pn2_fp_k, lds)) return -2;
  hipLaunchKernelGGL(pn2_fp_k, dim3((unsigned)gx, (unsigned)B), dim3(MT), (size_t)lds, (hipStream_t)stream, sparse_feature,
                     index, weight, dense_feature, params, ch, C2, C1, N2, N1, rs, out, status);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int mvk_pn2_fa_fwd(const float* feature_2d, int64_t stride_image, int64_t stride_channel, int64_t stride_pixel,
                              const float* image_xyz, const float* points, const int64_t* index, const int64_t* lengths,
                              const float* params, const int* widths_host, int n_layers, int B, int nv, int C, int64_t HW,
                              int64_t N, int K, int use_relation, int reduce, float* out, void* stream) {
  Chain ch;
  if (make_chain("pn2_fa_fwd", params, widths_host, n_layers, 1, &ch)) return -1;
  MVK_REQUIRE(K >= 1 && K <= 128, "pn2_fa_fwd: K = %d neighbours (1 .. 128 are supported)", K);
  MVK_REQUIRE(B >= 0 && B < 65536 && nv >= 1 && C >= 1 && HW >= 1 && N >= 0 && N < ((int64_t)1 << 31) &&
                  (int64_t)nv * HW < ((int64_t)1 << 31),
              "pn2_fa_fwd: bad sizes B=%d nv=%d C=%d HW=%lld N=%lld", B, nv, C, (long long)HW, (long long)N);
  MVK_REQUIRE(reduce == 0 || reduce == 1, "pn2_fa_fwd: reduce = %d (0 sum, 1 max)", reduce);
  MVK_REQUIRE(ch.width[0] == C + (use_relation ? 4 : 0), "pn2_fa_fwd: widths[0] = %d, the input rows hold %d values",
              ch.width[0], C + (use_relation ? 4 : 0));
  const int rs = pick_rshift(ch, AUX_FA, (int64_t)B * N * K, K);
  const int R = 1 << rs;
  MVK_REQUIRE(K <= R, "pn2_fa_fwd: widths %d, %d, %d, %d leave no room in LDS for a tile of K = %d rows", ch.width[0],
              ch.width[1], ch.width[2], ch.width[3], K);
  if (B == 0 || N == 0) return 0;
  MVK_REQUIRE(feature_2d && image_xyz && points && index && params && out, "pn2_fa_fwd: null operand");
  const int G = R / K;
  const int64_t gx = cdiv64(N, G), lds = lds_bytes(ch, R, AUX_FA);
  MVK_REQUIRE(gx < ((int64_t)1 << 31), "pn2_fa_fwd: too many points");
  if (allow_lds(pn2_fa_k, lds)) return -2;
  hipLaunchKernelGGL(pn2_fa_k, dim3((unsigned)gx, (unsigned)B), dim3(MT), (size_t)lds, (hipStream_t)stream, feature_2d,
                     stride_image, stride_channel, stride_pixel, image_xyz, points, index, lengths, params, ch, C, nv, (int)HW,
                     N, K, rs, G, reduce, out);
  MVK_CHECK_HIP(hipGetLastError());
  return 0;
}
