/* Third header of libmvkpconv.so: the training batches of the MVPNet baseline, built on the device from scenes that
 * are resident in HBM, B items at a time (csrc/train_inputs.hip; reference: mvpnet/data/scannet_2d3d.py:323-416,
 * ScanNet2D3DChunks.__getitem__, with get_rgbd_data, :191-321).
 *
 * include/mvkpconv.h stays the declaration of ABI 9 and include/mvkpconv_scene.h the declaration of the whole-scene
 * inputs; neither is touched. This header follows their style (one extern "C" block, functions and #define constants
 * only, every function ends in `void* stream`, returns 0 or a negative code with the text in mvk_last_error) and is
 * read by the same parser (_lib.parse_header -> TRAIN_FUNCTIONS).
 *
 * Common rules: every pointer is a device address. Sizes of 2^31 or more are refused. An empty problem (no item, no
 * try, no point to draw, no pixel) returns 0 without a launch. Nothing is read back to the host and nothing waits.
 * Integer arithmetic, float32 or float64 evaluated in the written order (-ffp-contract=off). Every kernel gives whole
 * workgroups to one item; the only atomics are integer counters, summed in LDS first.
 *
 * RESIDENT SCENES. S scenes lie one after another in
 *   points [P,3] f32, labels [P] int64 (training classes; negative = unlabeled), base_point_ind [NB] int64 (scene-local
 *   point numbers), bits [NW] 32-bit words (each scene's mvk_overlap_pack rows [num_frames][ceil(num_base / 32)]),
 *   depth [F,h,w] uint16 millimetres, images [F,h,w,3] f32, poses [F,4,4] f32, cam_inv [S,9] f64 (inverse intrinsics)
 * and are described by scenes [S,8] int64:
 *   point_off, num_points, base_off, num_base, frame_off, num_frames, bits_off (in words), 0.
 * Every entry point takes the table with the totals P, NB, F, NW and checks an item's row against them on the device:
 * an item whose scene_id lies outside [0, S), or whose row leaves the totals or the capacities below, is an EMPTY item
 * (no point, zeros, frame 0) -- never an access outside the buffers. */
#ifndef MVKPCONV_TRAIN_H
#define MVKPCONV_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most tries of mvk_train_chunk_pick (the reference makes 10) */
#define MVK_TRAIN_MAX_TRIES 32
/* points per workgroup of mvk_train_chunk_pick; its block_counts hold B * ceil(max_points / MVK_TRAIN_PICK_TILE) ints */
#define MVK_TRAIN_PICK_TILE 1024
/* positions per pass of mvk_train_chunk_resample's one workgroup per item */
#define MVK_TRAIN_RESAMPLE_STRIDE 1024

/* scannet_2d3d.py:340-371. Item b crops scene scene_id[b] ([B] int64) around T candidate centres: centers [B,T] int64
 * are scene-local point numbers that the CALLER drew (the reference draws one per try and stops at the first success:
 * given the same draws the result is the same; the generator's stream is not reproduced). For try t, in float32 and
 * in this order: lo = (c - 0.5f * size) - margin, hi = (c + 0.5f * size) + margin per axis, c the centre's xy; a point
 * is inside when x >= lo.x && x <= hi.x && y >= lo.y && y <= hi.y. cnt[t] = points inside, lab[t] = those with
 * label >= 0, both counted for all T tries in one pass over the scene. A centre outside [0, num_points) counts nothing.
 * chosen = the first t with cnt > 0 && (double)lab / (double)cnt >= chunk_thresh, else -1 = the whole scene, whose
 * lo / hi are the scene's min / max xy with the margin applied.
 * counts [B,T,2] int32 (cnt, lab); chosen [B] int32; box [B,4] f32 (lo.x, lo.y, hi.x, hi.y); the chunk's row = the
 * GLOBAL indices point_off + i of its points, ascending, at rows[row_off[b] ..) with row_len [B] int64 entries. row_off
 * [B] int64: the running sum of the items' num_points (the row's capacity); a row is cut to [0, total).
 * max_points: the largest num_points among the items' scenes (it sizes the grid; a larger scene is an empty item).
 * block_counts: B * ceil(max_points / MVK_TRAIN_PICK_TILE) ints of scratch. */
int mvk_train_chunk_pick(const float* points, const int64_t* labels, int64_t P, const int64_t* scenes, int S, int64_t NB,
                         int64_t F, int64_t NW, const int64_t* scene_id, const int64_t* centers, int B, int T,
                         float size_x, float size_y, float margin_x, float margin_y, double chunk_thresh,
                         int64_t max_points, const int64_t* row_off, int64_t total, int32_t* block_counts,
                         int32_t* counts, int32_t* chosen, float* box, int64_t* rows, int64_t* row_len, void* stream);

/* The library's own rule for scannet_2d3d.py:374-381 (NumPy's Mersenne draws of a count that only the device knows
 * cannot be repeated without reading it back). seeds [B] int64 from the caller; key_bits in 1..32. Mod 2^32:
 *   mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   draw(i) = mix32(lo32(seed) ^ mix32(hi32(seed) + i * 0x9e3779b9));  key(i) = draw(i) >> (32 - key_bits)
 * With nc = row_len[b]: nc >= nb_pts takes the nb_pts positions that come first in the order (key, position) -- a
 * uniformly drawn subset -- and writes them in ASCENDING position (the reference's order is a random permutation);
 * nc < nb_pts writes positions 0 .. nc-1 and then the pads (uint64(draw(nc + j)) * nc) >> 32, j = 0 ...
 * sample_pos [B,nb_pts] int32 (positions in the row), sample_rows [B,nb_pts] int64 = rows[row_off[b] + position]; an
 * empty row gives -1 in both. One workgroup per item: a radix select over the key, then an ordered compaction in
 * passes of MVK_TRAIN_RESAMPLE_STRIDE positions; keys are recomputed, never stored. */
int mvk_train_chunk_resample(const int64_t* rows, int64_t total, const int64_t* row_off, const int64_t* row_len,
                             const int64_t* seeds, int B, int64_t nb_pts, int key_bits, int64_t* sample_rows,
                             int32_t* sample_pos, void* stream);

/* mvk_chunk_select_frames (same tie rule, same behaviour once nothing is left) with item b reading ITS scene's bit rows
 * and base_point_ind: base point j belongs to the chunk when point_off + base_point_ind[base_off + j] is found in the
 * item's row (ascending, distinct: mvk_train_chunk_pick's, before the resample). sel [B,nv] int32, scene-local.
 * max_base / max_frames: the largest num_base / num_frames of the table (they size the LDS); refused above
 * MVK_SCENE_MAX_BASE / MVK_SCENE_MAX_FRAMES of mvkpconv_scene.h (524288 / 4096). */
int mvk_train_select_frames(const int32_t* bits, int64_t NW, const int64_t* base_point_ind, int64_t NB,
                            const int64_t* scenes, int S, int64_t P, int64_t F, const int64_t* scene_id,
                            const int64_t* rows, int64_t total, const int64_t* row_off, const int64_t* row_len, int B,
                            int nv, int64_t max_base, int64_t max_frames, int32_t* sel, void* stream);

/* mvk_chunk_unproject for items of different scenes: view v of item b is frame frame_off + sel[b,v], unprojected with
 * the item's cam_inv row by csrc/unproject.h's expression. valid = z_cam > 0 && x > (double)box[0] - 0.1 &&
 * x < (double)box[2] + 0.1 && y > (double)box[1] - 0.1 && y < (double)box[3] + 0.1, strict, in float64 (box [B,4] f32
 * of mvk_train_chunk_pick; scannet_2d3d.py:274-281 as NumPy 1.x evaluates it).
 * flips [B,nv] uint8 (may be null): where set, output pixel (r, c) of that view is source pixel (r, w-1-c) in keys,
 * image_xyz, image_mask and images_out alike (:293-296). rot [B,9] f64 row-major (may be null): image_xyz is rounded to
 * float32 first and then m[r][0]*x + m[r][1]*y + m[r][2]*z in float64, left to right, rounded to float32 (:400-409);
 * keys stay unrotated, as the reference's k-NN precedes its rotation.
 * keys [B, nv*h*w, 3] f64; image_xyz [B,nv,h,w,3] f32; image_mask [B,nv,h,w] uint8 0/1; images_out [B,nv,3,h,w] f32;
 * num_valid [B] int32 (zeroed here). A sel entry outside [0, num_frames) gives zeros and no valid pixel. */
int mvk_train_unproject(const int32_t* sel, const int64_t* scene_id, int B, int nv, const int64_t* scenes, int S,
                        int64_t P, int64_t NB, int64_t F, int64_t NW, const uint16_t* depth, const float* images_in,
                        const float* poses, const double* cam_inv, int h, int w, const float* box,
                        const uint8_t* flips, const double* rot, double* keys, float* image_xyz, uint8_t* image_mask,
                        float* images_out, int32_t* num_valid, void* stream);

/* The batch's rows: points_out [B,3,nb_pts] f32 = queries [B*nb_pts,3] f32 (mvk_chunk_knn_many's, the sampled points)
 * rotated by rot [B,9] f64 with mvk_train_unproject's rule (null: copied), and seg_label [B,nb_pts] int64 =
 * labels[sample_rows[b,j]], -100 where sample_rows lies outside [0, P). */
int mvk_train_batch_rows(const float* queries, const int64_t* labels, int64_t P, const int64_t* sample_rows,
                         const double* rot, int B, int64_t nb_pts, float* points_out, int64_t* seg_label,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVKPCONV_TRAIN_H */
