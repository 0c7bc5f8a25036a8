"""Training batches of the MVPNet baseline built on the device from scenes resident in HBM (not in the reference;
DESIGN.md 7q).

What ``train_mvpnet_3d.py`` feeds the network is ``ScanNet2D3DChunks.__getitem__`` (mvpnet/data/scannet_2d3d.py:323-416
with ``get_rgbd_data``, :191-321): per item ten tries at a random xy crop of the scene, a resample to nb_pts points, a
greedy frame choice, num_rgbd_frames unprojections and a ball tree, all NumPy in DataLoader workers. Here the scenes lie
in HBM once and a batch of B items from B scenes is a fixed handful of launches (csrc/train_inputs.hip and the k-NN of
csrc/scene_inputs.hip) behind one small upload, with nothing read back:

* ``TrainScenes``        the resident set: every scene's points, labels, base points, overlap bit rows and frames, one
                         after another, and the table that says where each scene lies
* ``train_chunk_batch``  the dict a collated reference batch has, plus 'chunk_try' and 'num_valid_pixels'

Two deliberate differences from the reference, both documented in DESIGN.md 7q:

* the host draws every random number up front -- ``tries`` centres per item where the reference draws one per try and
  stops at the first success. Given the same centres the crop is the reference's; the generator's stream is not.
* the resample is the library's own rule (include/mvkpconv_train.h: a hash of a per-item seed and the position). A
  chunk of at least nb_pts points gives a uniformly drawn subset in ASCENDING point order where the reference's
  ``np.random.choice`` gives a random permutation; a smaller chunk gives itself and hashed pads.

Colour jitter, loading and resizing the images, normalising them and mapping raw labels to training classes stay the
caller's: 'images' are taken as the float32 tensors the network is to see and 'seg_label' as training classes
(negative = unlabeled). The module is opt-in; nothing else of the drop-in uses it."""
import numpy as np
import torch

try:
    from .._native import ops
    from .whole_scene_inputs import SceneFrames, _in_hbm
except ImportError:  # dropin/ put on sys.path directly
    from _native import ops
    from mvpnet.whole_scene_inputs import SceneFrames, _in_hbm


class TrainScenes(object):
    """The resident training set. ``scenes``: a list of dicts with the keys of ``SceneFrames`` -- 'depth' (nf, h, w)
    integer millimetres, 'images' (nf, h, w, 3), 'poses' (nf, 4, 4), 'base_point_ind' (nb,), 'pointwise_rgbd_overlap'
    (nb, nf) in HBM, 'cam_matrix' on the host, already rescaled to (h, w) -- plus 'points' (n, 3) float32 and 'seg_label'
    (n,) int64 training classes in HBM. All scenes share (h, w). A scene without a point or a frame is refused.

    The scenes are concatenated once (a copy: the list's own tensors can be dropped afterwards)."""

    def __init__(self, scenes):
        if not scenes:
            raise ValueError("TrainScenes: at least one scene expected")
        frames = [SceneFrames(s) for s in scenes]
        hw = {(f.h, f.w) for f in frames}
        if len(hw) != 1:
            raise ValueError("TrainScenes: every scene's frames must have the same (h, w), found %s" % sorted(hw))
        points, labels, table = [], [], np.zeros((len(scenes), 8), np.int64)
        at = [0, 0, 0, 0]
        for i, (s, f) in enumerate(zip(scenes, frames)):
            p = _in_hbm("scene['points']", s['points'])
            if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != 3:
                raise RuntimeError("TrainScenes: points must be a float32 (num_points, 3) tensor")
            lab = _in_hbm("scene['seg_label']", s['seg_label'])
            if lab.dtype != torch.int64 or tuple(lab.shape) != (p.shape[0],):
                raise RuntimeError("TrainScenes: seg_label must be an int64 (num_points,) tensor")
            if p.shape[0] < 1 or f.num_frames < 1:
                raise ValueError("TrainScenes: scene %d has no point or no frame" % i)
            points.append(p)
            labels.append(lab)
            words = f.num_frames * ((f.num_base + 31) // 32)
            table[i] = (at[0], p.shape[0], at[1], f.num_base, at[2], f.num_frames, at[3], 0)
            at = [at[0] + p.shape[0], at[1] + f.num_base, at[2] + f.num_frames, at[3] + words]
        device = points[0].device
        cam_inv = np.stack([f.cam_inv.reshape(9) for f in frames])
        self.resident = ops.TrainResident(
            torch.cat(points).contiguous(), torch.cat(labels).contiguous(),
            torch.cat([f.base_point_ind for f in frames]).contiguous(),
            torch.cat([f.overlap_bits.reshape(-1) for f in frames]).contiguous(),
            torch.cat([f.depth16 for f in frames]).contiguous(), torch.cat([f.images for f in frames]).contiguous(),
            torch.cat([f.poses for f in frames]).contiguous(), torch.from_numpy(cam_inv).to(device), table)
        self.num_scenes = len(scenes)
        self.num_points = table[:, 1].copy()
        self.h, self.w = frames[0].h, frames[0].w


def z_rotation(angle_deg):
    """The 3 x 3 float64 matrix of a rotation about z by angle_deg degrees: scipy's
    ``Rotation.from_euler('z', a, degrees=True).as_matrix()`` when scipy is importable, else built from cos / sin."""
    try:
        from scipy.spatial.transform import Rotation
    except ImportError:
        c, s = np.cos(np.deg2rad(angle_deg)), np.sin(np.deg2rad(angle_deg))
        return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], np.float64)
    return np.ascontiguousarray(Rotation.from_euler('z', angle_deg, degrees=True).as_matrix(), dtype=np.float64)


def draw_items(num_points, nv, flip=0.0, z_rot=None, tries=10):
    """The host's draws for items of scenes with num_points[b] points, from the global NumPy generator, item by item in
    this order: ``np.random.randint(num_points[b], size=tries)`` (the centres), ``np.random.randint(2 ** 63,
    dtype=np.int64)`` (the resample seed), ``np.random.rand(nv) < flip`` when flip is set, ``np.random.uniform(*z_rot)``
    when z_rot is set. Returns (centers [B,tries] int64, seeds [B] int64, flips [B,nv] uint8 or None, angles [B] or None)."""
    B = len(num_points)
    centers, seeds = np.zeros((B, tries), np.int64), np.zeros(B, np.int64)
    flips = np.zeros((B, nv), np.uint8) if flip else None
    angles = np.zeros(B, np.float64) if z_rot else None
    for b, n in enumerate(num_points):
        centers[b] = np.random.randint(int(n), size=tries)
        seeds[b] = np.random.randint(2 ** 63, dtype=np.int64)
        if flip:
            flips[b] = np.random.rand(nv) < flip
        if z_rot:
            angles[b] = np.random.uniform(low=z_rot[0], high=z_rot[1])
    return centers, seeds, flips, angles


def train_chunk_batch(scenes, scene_ids, nb_pts, num_rgbd_frames, k=3, chunk_size=(1.5, 1.5), chunk_thresh=0.3,
                      chunk_margin=(0.2, 0.2), flip=0.0, z_rot=None, tries=10, draws=None, key_bits=32):
    """One training batch of B = len(scene_ids) items, item b a random chunk of scene scene_ids[b], as the reference's
    DataLoader collates ``ScanNet2D3DChunks(..., nb_pts, num_rgbd_frames, k, z_rot, flip, to_tensor=True)``:

    'points' (B, 3, nb_pts) f32, 'seg_label' (B, nb_pts) int64, 'images' (B, nv, 3, h, w) f32, 'image_xyz' (B, nv, h, w, 3)
    f32, 'image_mask' (B, nv, h, w) bool, 'knn_indices' (B, nb_pts, k) int64, and in addition 'chunk_try' (B,) int32 (the
    try that gave the chunk, -1 = the whole scene) and 'num_valid_pixels' (B,) int32. All in HBM.

    scenes: a ``TrainScenes``; flip: the probability of mirroring a view; z_rot: (low, high) degrees or None; tries: the
    candidate centres per item (10 reproduces the reference). The host draws with ``draw_items`` (its docstring gives the
    order), or takes ``draws`` = (centers, seeds, flips, angles) as that function returns them; everything goes up in one
    pinned upload. Nothing is read back and nothing waits for the device.

    An item with fewer than k valid pixels has -1 where no neighbour exists and 'num_valid_pixels' says so, as in
    ``whole_scene_inputs.group_rgbd_inputs``; the reference raises there. The caller decides when to look."""
    res = scenes.resident
    ids = np.asarray(scene_ids, dtype=np.int64).reshape(-1)
    B, nv, k, nb_pts = len(ids), int(num_rgbd_frames), int(k), int(nb_pts)
    if B < 1 or nb_pts < 1:
        raise ValueError("train_chunk_batch: at least one item and one point expected")
    if ids.min() < 0 or ids.max() >= scenes.num_scenes:
        raise ValueError("train_chunk_batch: scene_ids must lie in [0, %d)" % scenes.num_scenes)
    sizes = scenes.num_points[ids]
    centers, seeds, flips, angles = draw_items(sizes, nv, flip, z_rot, tries) if draws is None else draws
    rot = None if angles is None else np.stack([z_rotation(a) for a in angles]).reshape(B, 9)
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    T = centers.shape[1]
    flip_bytes = np.zeros(-(-B * nv // 8) * 8, np.uint8)
    if flips is not None:
        flip_bytes[:B * nv] = np.asarray(flips, np.uint8).reshape(-1)
    # one upload: scene_id | centers | seeds | row_off | sample offsets | rot as words | flips as words
    words = np.concatenate([ids, np.asarray(centers, np.int64).reshape(-1), np.asarray(seeds, np.int64), row_off[:B],
                            np.arange(B + 1, dtype=np.int64) * nb_pts,
                            (rot if rot is not None else np.zeros((B, 9))).astype(np.float64).reshape(-1).view(np.int64),
                            flip_bytes.view(np.int64)])
    staged = torch.empty((len(words),), dtype=torch.int64, pin_memory=True)
    staged.numpy()[:] = words
    meta = staged.to(res.points.device, non_blocking=True)
    at = [0]

    def take(n):
        at[0] += n
        return meta[at[0] - n:at[0]]

    sid_d, centers_d, seeds_d, row_off_d = take(B), take(B * T).view(B, T), take(B), take(B)
    samp_off_d = take(B + 1)
    rot_d = take(B * 9).view(torch.float64).view(B, 9)
    flips_d = take(len(flip_bytes) // 8).view(torch.uint8)[:B * nv].view(B, nv)

    _, chosen, box, rows, row_len = ops.train_chunk_pick(res, sid_d, centers_d, row_off_d, int(row_off[B]), chunk_size,
                                                         chunk_margin, chunk_thresh, max_points=int(sizes.max()))
    sample_rows, _ = ops.train_chunk_resample(rows, row_off_d, row_len, seeds_d, nb_pts, key_bits=key_bits)
    sel = ops.train_select_frames(res, sid_d, rows, row_off_d, row_len, nv)
    keys, image_xyz, image_mask, images, num_valid = ops.train_unproject(
        res, sel, sid_d, box, flips=flips_d if flips is not None else None, rot=rot_d if rot is not None else None)
    queries, knn = ops.chunk_knn_many(res.points, sample_rows.view(-1), samp_off_d[:B], samp_off_d,
                                      np.full(B, nb_pts, np.int64), keys, image_mask, k=k)
    points, seg_label = ops.train_batch_rows(queries, res.labels, sample_rows, rot=rot_d if rot is not None else None)
    return {'points': points, 'seg_label': seg_label, 'images': images, 'image_xyz': image_xyz, 'image_mask': image_mask,
            'knn_indices': knn.view(B, nb_pts, k), 'chunk_try': chosen, 'num_valid_pixels': num_valid}
