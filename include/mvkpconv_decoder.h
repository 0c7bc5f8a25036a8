/* Fifth header of libmvkpconv.so: the KPFCNN decoder's unary layers as two products, without the concatenation
 * (csrc/gemm.hip; reference: KPConv-PyTorch/models/architectures.py:334-335 -- closest_pool + torch.cat -- and the unary
 * block behind it, models/blocks.py:470-504). By linearity
 *
 *     cat([x_c[idx], skip]) . W^T  =  (x_c . W[:, :C1]^T)[idx]  +  skip . W[:, C1:]^T
 *
 * and with G_c[j] = sum of the gradient rows g[n] over the fine points n with idx[n] = j:
 *     dx_c = G_c . W[:, :C1]      d_skip = g . W[:, C1:]      dW = [ G_c^T . x_c | g^T . skip ]
 * so the upsampled half of every product runs at COARSE rows (a level keeps about 1/4.4 of the points).
 *
 * The other headers of the library are not touched: nothing they declare changes its meaning or its layout, so this is an
 * addition to ABI 9, not a new version. Same style (one extern "C" block, functions only, every launching function ends in
 * `void* stream`, returns 0 or a negative code with the text in mvk_last_error), read by the same parser
 * (_lib.parse_header -> DECODER_FUNCTIONS). All matrices row-major float32, every pointer a device address. */
#ifndef MVKPCONV_DECODER_H
#define MVKPCONV_DECODER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* C [M,N] = A [M,Kd] . B[:, col0:col0+Kd]^T for a row-major B [N, ldb] read in place (a column block of a wider weight
 * matrix, no copy), plus the optional row-gathered addend: row m gets + add_src[add_idx[m * add_stride], :]
 * (add_src [add_ns, N] dense; NULL: none; add_idx int32, or int64 when add_idx64 != 0; an index outside [0, add_ns) -- the
 * shadow row -- adds nothing). The addend goes in BEFORE the statistics, exactly once whatever the split of the reduction
 * (unsplit: the tile itself; atomic split: split 0; ordered split: the last arriver, after it has summed the slots).
 * bn_part / n_valid: the BatchNorm-statistics epilogue of mvk_gemm_f32_ex, and fin (a `const mvk_bn_finish*` of
 * mvkpconv.h, or NULL) its finish as in mvk_gemm_f32_bn; the plan is mvk_gemm_f32_plan(M, N, Kd, 0, bn_part != NULL):
 * zero-initialise C when that splits and no arena is set. */
int mvk_gemm_f32_nt_ldb_add(const float* A, const float* B, int64_t col0, int64_t ldb, float* C, int64_t M, int64_t N,
                            int64_t Kd, const float* add_src, const void* add_idx, int add_idx64, int64_t add_stride,
                            int64_t add_ns, float* bn_part, const int32_t* n_valid, const void* fin, void* stream);

/* Two NN products of DIFFERENT row counts in ONE launch: C0 [M0,N0] = A0 [M0,Kd] . B0 and C1 [M1,N1] = A1 [M1,Kd] . B1,
 * B0 / B1 [Kd, *] column blocks of row-major matrices whose rows are ldb floats apart (workgroups beyond a product's own
 * row tiles leave at once): dx_c at coarse rows beside d_skip at fine rows. mvk_gemm_f32_nn_pair_plan: out[0] = 1 when the
 * pair can share a launch (both outputs wider than 32 columns), out[1..2] = the splits of the two reductions
 * (zero-initialise an output whose split is > 1 unless an arena is set). */
int mvk_gemm_f32_nn_pair_plan(int64_t M0, int64_t N0, int64_t M1, int64_t N1, int64_t Kd, int* out /* [3] */);
int mvk_gemm_f32_nn_pair(const float* A0, const float* B0, float* C0, int64_t M0, int64_t N0, const float* A1,
                         const float* B1, float* C1, int64_t M1, int64_t N1, int64_t Kd, int64_t ldb, void* stream);

/* C[:, 0:N] = A^T . B (A [Kd,M], B [Kd,N]) into a column window of a wider matrix whose rows are ldc >= N floats apart;
 * split as mvk_gemm_f32_plan(M, N, Kd) says (zero-initialise the window when > 1 and no arena is set). Columns outside
 * the window are not touched. */
int mvk_gemm_f32_tn_ldc(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t Kd, int64_t ldc,
                        void* stream);

/* mvk_gemm_f32_tn_grouped_plan for records with an output leading dimension, {const float* A; const float* B; float* C;
 * int64 M, N, Kd, ldc;} (56 bytes): C_i is a column window of a wider matrix, rows ldc_i >= N_i floats apart -- two
 * products fill the two slabs of one weight gradient. Same table, same launch (mvk_gemm_f32_tn_grouped). */
int mvk_gemm_f32_tn_grouped_plan_ldc(const void* problems, int n, void* table_host, int* n_narrow, int64_t* wgs_narrow,
                                     int64_t* wgs_wide, int32_t* splits, void* stream);

#ifdef __cplusplus
}
#endif

#endif
