/* Second header of libmvkpconv.so: the inputs of the MVPNet whole-scene test, built on the device for G chunks at a
 * time (csrc/scene_inputs.hip; reference: mvpnet/data/scannet_2d3d.py:199-321, mvpnet/test_mvpnet_3d.py:153-158).
 *
 * include/mvkpconv.h stays the declaration of ABI 9 and is not touched by these entry points; this header follows its
 * style (one extern "C" block, the same few types, every function ends in `void* stream`, returns 0 or a negative code
 * with the text in mvk_last_error) and is read by the same parser (_lib.parse_header -> SCENE_FUNCTIONS).
 *
 * Common rules: every pointer is a device address unless its name ends in _host. Sizes of 2^31 or more are refused. An
 * empty problem (no chunk, no frame to choose, no pixel) returns 0 without a launch. Nothing is read back to the host
 * and nothing waits. Integer arithmetic or float64 evaluated in the written order (-ffp-contract=off); the only atomics
 * are integer counters, one per workgroup. */
#ifndef MVKPCONV_SCENE_H
#define MVKPCONV_SCENE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* capacity of mvk_chunk_select_frames: its mask of base points (64 KiB of bits) and its counts live in LDS */
#define MVK_SCENE_MAX_BASE 524288
#define MVK_SCENE_MAX_FRAMES 4096

/* overlap [nb, nf] uint8 / bool (pointwise_rgbd_overlap; any non-zero byte counts as true) -> packed, frame-major bit
 * rows [nf][ceil(nb / 32)] of 32-bit words: bit (b % 32) of word b / 32 of row f is set when base point b is seen by
 * frame f. Bits past nb are zero. Once per scene. */
int mvk_overlap_pack(const uint8_t* overlap, int64_t nb, int64_t nf, int32_t* packed, void* stream);

/* Greedy maximum coverage (scannet_2d3d.py:199-221, ScanNet_sphere_color.py:53-63) for G chunks in one launch, one
 * workgroup per chunk. Chunk g is the row rows[row_off[g] .. row_off[g] + row_len[g]) of a CSR of scene point indices
 * (rows [total] int64; row_off, row_len [G] int64). CONTRACT: every row is ascending and distinct, as
 * scene2chunks_legacy makes it (np.nonzero order) -- base point b belongs to the chunk when base_point_ind[b] (int64
 * [nb]) is found in the row by binary search. A row that leaves [0, total) is cut to it.
 * nv rounds: count[f] = base points of the chunk seen by frame f and not yet covered; the FIRST maximum is chosen (ties
 * go to the lower frame); its base points are covered. Once nothing is left every count is 0 and frame 0 is chosen
 * again and again, and a chunk without a base point chooses frame 0 nv times -- as the reference does.
 * sel [G, nv] int32. Refused: nb > MVK_SCENE_MAX_BASE, nf > MVK_SCENE_MAX_FRAMES, nf < 1. */
int mvk_chunk_select_frames(const int32_t* packed, int64_t nb, int64_t nf, const int64_t* base_point_ind,
                            const int64_t* rows, int64_t total, const int64_t* row_off, const int64_t* row_len, int G,
                            int nv, int32_t* sel, void* stream);

/* The chosen frames of G chunks unprojected, masked by the chunk's box and gathered, one launch over G * nv * h * w
 * pixels (rounded up to whole workgroups per chunk). sel [G, nv] int32 is read on the device. depth (nf,h,w) uint16
 * millimetres, images_in (nf,h,w,3) f32, poses (nf,4,4) f32, cam_inv_host [3,3] f64 (HOST; inverse intrinsics).
 * World coordinates: mvk_unproject_depth's expression in its order (csrc/unproject.h), so the same bits.
 * bounds [G,4] f64 (xlo, xhi, ylo, yhi): valid = z_cam > 0 && x > xlo && x < xhi && y > ylo && y < yhi, strict, in
 * float64 (scannet_2d3d.py:255-281).
 * keys [G, nv*h*w, 3] f64; image_xyz [G,nv,h,w,3] f32 = the rounded keys; image_mask [G,nv,h,w] uint8 0/1; images_out
 * [G,nv,3,h,w] f32; num_valid [G] int32 = valid pixels per chunk (zeroed here). A sel entry outside [0, nf) gives
 * zeros and no valid pixel. */
int mvk_chunk_unproject(const int32_t* sel, int G, int nv, const uint16_t* depth, const float* images_in,
                        const float* poses, int64_t nf, int h, int w, const double* cam_inv_host, const double* bounds,
                        double* keys, float* image_xyz, uint8_t* image_mask, float* images_out, int32_t* num_valid,
                        void* stream);

/* Workspace of mvk_chunk_knn_many for chunks of row_len_host[g] points and nk keys each: the largest
 * mvk_knn_workspace of the G calls, which run one after another in stream order. */
int64_t mvk_scene_inputs_workspace(const int64_t* row_len_host, int G, int64_t nk, int k);

/* The chunks' own points as queries and their exact float64 k-NN among the chunk's valid pixels: queries [sum, 3] f32
 * with queries[q_off[g] + j] = points[rows[row_off[g] + j]] (points [N,3] f32; an index outside [0, N) gives zeros),
 * then mvk_knn_f64 once per chunk on this stream (brute or pruned by its own host rule): queries of chunk g against
 * keys [G, nk, 3] f64 / key_valid [G, nk] uint8 of chunk g -> knn [sum, k] int64, flat pixel indices, -1 where a chunk
 * has fewer than k valid pixels. row_len_host / q_off_host: HOST copies [G] / [G+1] of row_len and of its running sum
 * (they size the launches); q_off [G+1] int64 is the running sum on the device. */
int mvk_chunk_knn_many(const float* points, int64_t N, const int64_t* rows, int64_t total, const int64_t* row_off,
                       const int64_t* q_off, const int64_t* row_len_host, const int64_t* q_off_host, int G,
                       const double* keys, const uint8_t* key_valid, int64_t nk, int k, float* queries, int64_t* knn,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* The group as the padded batch that collate_chunks builds: points_out [G, 3, n_max] f32 and knn_out [G, n_max, k]
 * int64. Column j of chunk g is the chunk's row r: r = j for j < row_len[g]; r = extras[extra_off[g] + j - row_len[g]]
 * for row_len[g] <= j < lengths[g] (the pad of a chunk below min_nb_pts, test_mvpnet_3d.py:153-158; extras int32,
 * extra_off [G+1] int64); zeros for lengths[g] <= j < n_max. An r outside [0, row_len[g]) gives zeros. */
int mvk_chunk_batch_rows(const float* queries, const int64_t* knn, const int64_t* q_off, const int64_t* row_len,
                         const int64_t* lengths, const int32_t* extras, const int64_t* extra_off, int G, int64_t n_max,
                         int k, float* points_out, int64_t* knn_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVKPCONV_SCENE_H */
