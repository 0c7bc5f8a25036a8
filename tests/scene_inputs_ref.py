"""NumPy restatements for the tests of csrc/scene_inputs.hip (the inputs of the MVPNet whole-scene test, G chunks at a
time): the greedy frame choice on packed words, the pixel mask, the layout of the padded batch, and the synthetic frames
the GPU tests share. Nothing here reads the reference tree.

The frame choice is integer arithmetic: count[f] = popcount(row_f & alive) summed over the words, the first maximum,
alive &= ~row_pick. The mask is a strict float64 comparison. The batch layout only copies."""
import numpy as np

PIXEL_MARGIN = 0.1


# -------------------------------------------------------------------------------------------------------- frame choice

def pack_overlap(overlap):
    """(nb, nf) bool -> frame-major bit rows [nf, ceil(nb / 32)] uint32: bit b % 32 of word b // 32; bits past nb zero."""
    overlap = np.asarray(overlap).astype(bool)
    nb, nf = overlap.shape
    W = (nb + 31) // 32
    padded = np.zeros((W * 32, nf), bool)
    padded[:nb] = overlap
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return np.ascontiguousarray((padded.T.reshape(nf, W, 32).astype(np.uint64) * weights).sum(axis=2).astype(np.uint32))


def pack_mask(mask):
    """(nb,) bool -> [ceil(nb / 32)] uint32 words."""
    return pack_overlap(np.asarray(mask).reshape(-1, 1))[0]


def popcount(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).reshape(words.shape + (32,)).sum(axis=-1).astype(np.int64)


def select_packed(packed, alive, num_frames):
    """Greedy maximum coverage on packed words: packed [nf, W] uint32, alive [W] uint32 (the chunk's base points)."""
    alive, out = alive.copy(), []
    for _ in range(num_frames):
        counts = popcount(packed & alive[None, :]).sum(axis=1)
        f = int(np.argmax(counts))                          # the first maximum
        out.append(f)
        alive &= ~packed[f]
    return out


def base_points_of_chunk(base_point_ind, chunk_row):
    """(nb,) bool: base point b lies in the chunk (chunk_row ascending and distinct: a binary search)."""
    chunk_row = np.asarray(chunk_row)
    if len(chunk_row) == 0:
        return np.zeros(len(base_point_ind), bool)
    at = np.minimum(np.searchsorted(chunk_row, base_point_ind), len(chunk_row) - 1)
    return chunk_row[at] == base_point_ind


def select_frames_of_chunk(overlap, base_point_ind, chunk_row, num_frames):
    return select_packed(pack_overlap(overlap), pack_mask(base_points_of_chunk(base_point_ind, chunk_row)), num_frames)


def select_frames_table(overlap, num_frames):
    """The reference's loop (ScanNet_sphere_color.py:53-63) on the bool table itself."""
    overlap, out = np.asarray(overlap).astype(bool).copy(), []
    for _ in range(num_frames):
        f = int(overlap.sum(0).argmax())
        out.append(f)
        overlap[overlap[:, f]] = False
    return out


# ---------------------------------------------------------------------------------------------------------------- mask

def box_bounds(chunk_box):
    """(xlo, xhi, ylo, yhi) float64 of a chunk's (x1, y1, z1, x2, y2, z2), as chunk_rgbd_inputs forms them."""
    box = np.asarray(chunk_box, dtype=np.float64)[[0, 1, 3, 4]]
    return np.array([float(box[0] - PIXEL_MARGIN), float(box[2] + PIXEL_MARGIN), float(box[1] - PIXEL_MARGIN),
                     float(box[3] + PIXEL_MARGIN)], np.float64)


def pixel_mask(xyz, depth_valid, bounds):
    """xyz (..., 3) float64 world coordinates, depth_valid (...) bool (z_cam > 0): strictly inside the bounds, in float64."""
    assert xyz.dtype == np.float64
    x, y = xyz[..., 0], xyz[..., 1]
    return depth_valid & (x > bounds[0]) & (x < bounds[1]) & (y > bounds[2]) & (y < bounds[3])


# --------------------------------------------------------------------------------------------------------------- batch

def pad_extras(sizes, min_nb_pts):
    """The pad rows of every chunk below min_nb_pts, drawn in chunk order from the global NumPy generator
    (test_mvpnet_3d.py:153-158)."""
    return [np.random.randint(nc, size=min_nb_pts - nc) if nc < min_nb_pts else np.zeros(0, np.int64) for nc in sizes]


def batch_layout(chunk_points, chunk_knn, extras):
    """points [G, 3, n_max] f32, knn_indices [G, n_max, k] int64, lengths [G]: chunk g's rows (chunk_points[g] (nc, 3),
    chunk_knn[g] (nc, k)), then its rows extras[g], then zeros."""
    lengths = np.array([len(p) + len(e) for p, e in zip(chunk_points, extras)], np.int64)
    n_max, k = int(lengths.max()), chunk_knn[0].shape[1]
    points = np.zeros((len(chunk_points), 3, n_max), np.float32)
    knn = np.zeros((len(chunk_points), n_max, k), np.int64)
    for g, (p, q, e) in enumerate(zip(chunk_points, chunk_knn, extras)):
        r = np.concatenate([np.arange(len(p)), np.asarray(e, np.int64)])
        points[g, :, :len(r)] = p[r].T
        knn[g, :len(r)] = q[r]
    return points, knn, lengths


# -------------------------------------------------------------------------------------------------------------- frames

def synthetic_frames(points, nf=5, h=12, w=16, nb=400, seed=21):
    """Host arrays of the frames that tests/test_chunk_gpu.py builds: depth frames looking along +z from below the scene,
    each shifted in xy, so pixels land all over the scene's xy extent. One frame has no valid depth at all, another has
    holes."""
    rng = np.random.default_rng(seed)
    cam = np.array([[6.0, 0, w / 2], [0, 6.0, h / 2], [0, 0, 1]], np.float32)
    depth = rng.integers(900, 2100, size=(nf, h, w)).astype(np.int16)
    depth[1] = 0
    depth[2][rng.random((h, w)) < 0.3] = 0
    poses = np.tile(np.eye(4, dtype=np.float32), (nf, 1, 1))
    centre = (points.max(0) + points.min(0)) / 2
    for f in range(nf):
        poses[f, :3, 3] = (centre[0] + 0.4 * (f - 2), centre[1] - 0.3 * (f - 2), -1.0)
    return {"depth": depth, "images": rng.standard_normal((nf, h, w, 3)).astype(np.float32), "poses": poses,
            "cam_matrix": cam, "base_point_ind": np.sort(rng.choice(len(points), nb, replace=False)).astype(np.int64),
            "pointwise_rgbd_overlap": rng.random((nb, nf)) < 0.3}
