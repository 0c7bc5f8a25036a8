/* Fourth header of libmvkpconv.so: the sphere batches of the KPFCNN networks, built on the device
 * (csrc/sphere_inputs.hip; reference: KPConv-PyTorch/datasets/ScanNet_sphere_color.py:494-876, potential_item, with
 * get_rgbd_data, :352-474).
 *
 * The other headers of the library are not touched and not named here. This one follows their style (one extern "C" block,
 * functions and #define constants only, every launching function ends in `void* stream`, returns 0 or a negative code with
 * the text in mvk_last_error) and is read by the same parser (_lib.parse_header -> SPHERE_FUNCTIONS).
 *
 * Common rules: every pointer is a device address. An empty problem returns 0 without a launch. Nothing is read back to
 * the host and nothing waits. Every launch geometry follows from the sizes the HOST passes; the lengths of the items exist
 * only on the device. Float64 evaluated in the written order (-ffp-contract=off). */
#ifndef MVKPCONV_SPHERE_H
#define MVKPCONV_SPHERE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most items of one mvk_knn_f64_ragged call (one workgroup plans them) */
#define MVK_KNN_RAGGED_MAX_ITEMS 1024

/* Bytes of workspace of mvk_knn_f64_ragged for B items, cap query slots, nk keys per item and k neighbours; -1 when a
 * size is refused. */
int64_t mvk_knn_ragged_workspace(int B, int64_t cap, int64_t nk, int k);

/* The exact float64 k-NN of B items in a fixed number of launches: the result is the library's single-item k-NN
 * (float64 squared distance in three rounded products and sums, neighbours ordered by (d2, index)) on every item alone, bit
 * for bit.
 * points [N,3] f32; rows [cap] int64; q_off [B+1] int64 ON THE DEVICE, non-decreasing: the query at slot s in
 * [q_off[b], q_off[b+1]) belongs to item b and is points[rows[s]], or (0,0,0) when rows[s] lies outside [0, N).
 * q_off is read clamped to [0, cap] and made non-decreasing on the device (a running maximum), so no value of it leads to
 * an access outside the buffers. keys [B,nk,3] f64 and key_valid [B,nk] uint8 (may be null: all valid): item b's keys.
 * knn [cap,k] int64: the key's number in its item, -1 in the columns for which the item has no valid key left, -1 in
 * every slot at or past q_off[B]. queries_out [cap,3] f32 (may be null): the gathered queries, zeros past q_off[B].
 * k in 1..8; B in 1..MVK_KNN_RAGGED_MAX_ITEMS; cap + B * nk < 2^30.
 * Every item goes down the pruned search (32^3 Morton grid per item, 64-key tiles with outward-rounded boxes, workgroups
 * of 64 consecutive sorted queries of one item): no host rule looks at a length. Launches: one fill, plan, count, scan
 * (2 workgroups per item), scatter, boxes, search. */
int mvk_knn_f64_ragged(const float* points, int64_t N, const int64_t* rows, int64_t cap, const int64_t* q_off, int B,
                       const double* keys, const uint8_t* key_valid, int64_t nk, int k, int64_t* knn,
                       float* queries_out, void* workspace, int64_t workspace_bytes, void* stream);

/* RESIDENT SCENES. The layout of the MVPNet training batches (S scenes one after another in points [P,3] f32, labels [P]
 * int64, base_point_ind [NB] int64, bits [NW] 32-bit words, depth / images / poses of F frames, cam_inv [S,9] f64,
 * described by scenes [S,8] int64 = point_off, num_points, base_off, num_base, frame_off, num_frames, bits_off, 0), with
 * the points being the dl-subsampled clouds, extended by
 *   colors [P,3] f32, pot_points [PP,3] f32 (the coarse potential points of all scenes back to back), potentials [PP] f64,
 *   pots [S,2] int64 = pot_off, num_pot, min_potentials [S] f64 and argmin_potentials [S] int64 (scene-local).
 * Every kernel checks a slot's rows against the totals P, NB, F, NW, PP on the device: a slot whose cloud_ind lies outside
 * [0, S), or whose row leaves the totals, is an EMPTY slot (no point, zeros, frame 0) -- never an access outside the
 * buffers. Sizes of 2^31 or more are refused. */

/* points per workgroup of mvk_sphere_members; its block_counts hold B_max * ceil(max_points / MVK_SPHERE_TILE) ints */
#define MVK_SPHERE_TILE 1024
/* the most sphere slots of one batch */
#define MVK_SPHERE_MAX_SLOTS 1024

/* ScanNet_sphere_color.py:556-602 with the stop rule :690-694 for up to B_max spheres in ONE launch of one workgroup
 * (the picks depend on each other). Per pick:
 *   cloud = the lowest index of the smallest min_potentials; point = argmin_potentials[cloud]; the centre is potential
 *   point pot_off + point (float32, promoted to float64 for the tests below);
 *   potentials[i] of that cloud += the Tukey weight of every potential point with float64 rdist <= in_radius^2 -- the
 *   arithmetic of mvk_tukey_update, from one shared expression; min_potentials / argmin_potentials [cloud] = the new
 *   minimum, the lowest index among equals;
 *   n = the number of the scene's points with float64 rdist <= in_radius^2 (the membership test of mvk_ball_query);
 *   the slot is recorded, batch_n += n, and the loop ends once batch_n > batch_limit (the sphere that crosses the limit is
 *   part of the batch).
 * A cloud whose rows leave the totals (or whose arg-min leaves its potential points) ends the loop without a slot. Slots
 * never reached get cloud_ind = point_ind = -1, a zero centre and length 0, and leave the potentials untouched.
 * cloud_ind, point_ind [B_max] int64; centers [B_max,3] f32; lengths [B_max] int32; num_spheres [1] int32. */
int mvk_sphere_pick(const float* pot_points, int64_t PP, double* potentials, const int64_t* pots, double* min_potentials,
                    int64_t* argmin_potentials, const float* points, int64_t P, const int64_t* scenes, int S, int64_t NB,
                    int64_t F, int64_t NW, double in_radius, int64_t batch_limit, int B_max, int64_t* cloud_ind,
                    int64_t* point_ind, float* centers, int32_t* lengths, int32_t* num_spheres, void* stream);

/* The rows of all slots at once: slot b's row holds the GLOBAL indices point_off + i, ascending, of the points of scene
 * cloud_ind[b] with float64 rdist <= radius^2 around centers[b] (mvk_ball_query's test), at rows[q_off[b] .. q_off[b+1]).
 * Three launches: tile counts, one workgroup's exclusive scan that also writes q_off [B_max+1] int64 on the DEVICE, and
 * the scatter. q_off is cut to cap: rows that do not fit cap are dropped, never written, and status[0] is set to 1
 * (status [1] int32, otherwise left as it is: the caller zeroes it).
 * max_points: the largest num_points of the table (it sizes the grid; a larger scene is an empty slot). */
int mvk_sphere_members(const float* points, int64_t P, const int64_t* scenes, int S, int64_t NB, int64_t F, int64_t NW,
                       const int64_t* cloud_ind, const float* centers, int B_max, double radius, int64_t max_points,
                       int64_t cap, int32_t* block_counts, int64_t* rows, int64_t* q_off, int32_t* status, void* stream);

/* The greedy frame choice (ScanNet_sphere_color.py:361-376) of every slot on its own scene, one workgroup per slot, by the
 * integer arithmetic and tie rule of the library's other frame choices (csrc/select_frames.h): base point j takes part
 * when point_off + base_point_ind[base_off + j] is found in the slot's MASK row mask_rows[mask_off[b] .. mask_off[b+1])
 * -- mvk_sphere_members with radius in_radius + mask_margin. sel [B_max,nv] int32, scene-local. An empty slot chooses
 * frame 0 nv times. max_base / max_frames: the largest num_base / num_frames of the table (they size the LDS); refused
 * above 524288 / 4096. */
int mvk_sphere_select_frames(const int32_t* bits, int64_t NW, const int64_t* base_point_ind, int64_t NB,
                             const int64_t* scenes, int S, int64_t P, int64_t F, const int64_t* cloud_ind,
                             const int64_t* mask_rows, int64_t cap, const int64_t* mask_off, int B_max, int nv,
                             int64_t max_base, int64_t max_frames, int32_t* sel, void* stream);

/* One launch over cap rows (ScanNet_sphere_color.py:605-616, :657-670 with datasets/common.py:316). Row i of slot b
 * (q_off[b] <= i < q_off[b+1]) is world point p = points[rows[i]], centre c = centers[b]:
 *   x = (float)((double)p - (double)c)                                  (:605: float64 difference, rounded once)
 *   aug_j = ((x0 * R[0][j] + x1 * R[1][j]) + x2 * R[2][j]) * scale[j] + noise[i][j], in float32 in this order
 *           (R [B_max,9] f32 row-major and scale [B_max,3] f32 from the caller; noise [cap,3] f32 may be null)
 *   world_j = (float)((double)aug_j + (double)c_j)                      (:664, :670; column 2 is the height feature)
 *   feat_aggre_points = p; colors_out = colors[rows[i]] * keep_color[b] (keep_color [B_max] f32, 0 or 1);
 *   labels_out = labels[rows[i]]; input_inds = rows[i] - point_off (scene-local);
 *   knn_stacked = knn[i] + b * npix, -1 staying -1 (knn [cap,k] int64; npix = nv * h * w).
 * A row of no slot, a row of an empty slot and a rows entry outside the slot's scene give zeros, and -1 in input_inds
 * and knn_stacked. aug_points, world, feat_aggre_points, colors_out [cap,3] f32; labels_out, input_inds [cap] int64. */
int mvk_sphere_batch_rows(const float* points, const float* colors, const int64_t* labels, int64_t P,
                          const int64_t* scenes, int S, int64_t NB, int64_t F, int64_t NW, const int64_t* cloud_ind,
                          const float* centers, const int64_t* rows, int64_t cap, const int64_t* q_off, int B_max,
                          const float* R, const float* scale, const float* noise, const float* keep_color,
                          const int64_t* knn, int k, int64_t npix, float* aug_points, float* world,
                          float* feat_aggre_points, float* colors_out, int64_t* labels_out, int64_t* knn_stacked,
                          int64_t* input_inds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVKPCONV_SPHERE_H */
