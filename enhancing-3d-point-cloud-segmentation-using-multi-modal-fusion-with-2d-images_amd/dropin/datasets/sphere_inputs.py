"""Sphere batches of the KPFCNN networks built on the device from scenes resident in HBM (not in the reference;
DESIGN.md 7r).

What ``train_ScanNet_sphere.py`` feeds the networks is ``ScanNetDataset.potential_item`` (datasets/
ScanNet_sphere_color.py:494-876 with ``get_rgbd_data``, :352-474): per sphere the arg-min of the sampling potentials and
their Tukey update, two ``query_radius`` calls, a greedy frame choice on the base points of the slightly larger mask
sphere, num_rgbd_frames unprojections, a ball tree for the 3-NN pixels and ``augmentation_transform``, until the batch
holds more than ``batch_limit`` points -- NumPy and scikit-learn in DataLoader workers. Here the scenes lie in HBM once
and a batch of up to ``max_spheres`` spheres is a fixed number of launches (csrc/sphere_inputs.hip) behind one small
upload, with nothing read back:

* ``SphereScenes``    the resident set: ``mvpnet.train_inputs.TrainScenes``' layout plus colours, the coarse potential
                      points and the potentials
* ``sphere_batch``    a dict of HBM tensors over ``cap`` rows and ``max_spheres`` slots
* ``to_sphere_batch`` the one read-back (the number of spheres and their lengths), the pyramid, the ``SphereBatch``

Two deliberate differences from the reference, both documented in DESIGN.md 7r:

* the host draws every random number up front, for all ``max_spheres`` slots, where the reference draws per sphere it
  actually makes. Given the same draws the batch is the reference's; the generator's stream is not.
* the augmentation noise is an input tensor in HBM (``noise``, [cap, 3] float32, None = no noise): the reference's
  ``randn(n, 3)`` needs the sphere's size, which only the device knows. Row i's noise is added to stacked point i.

Inside a sphere the points are in ASCENDING point order (the reference's order is its KD-tree's). Colour jitter, loading
and resizing the images, normalising them and mapping labels stay the caller's. The module is opt-in; nothing else of
the drop-in uses it."""
import numpy as np
import torch

try:
    from .._native import ops
    from ..kernels.kernel_points import create_3D_rotations
    from ..mvpnet.whole_scene_inputs import SceneFrames, _in_hbm
    from .common import segmentation_inputs_sphere, SphereBatch
except ImportError:  # dropin/ put on sys.path directly
    from _native import ops
    from kernels.kernel_points import create_3D_rotations
    from mvpnet.whole_scene_inputs import SceneFrames, _in_hbm
    from datasets.common import segmentation_inputs_sphere, SphereBatch


class SphereScenes(object):
    """The resident set. ``scene_dicts``: a list of dicts with the keys of ``SceneFrames`` -- 'depth' (nf, h, w) integer
    millimetres, 'images' (nf, h, w, 3), 'poses' (nf, 4, 4), 'base_point_ind' (nb,), 'pointwise_rgbd_overlap' (nb, nf) in
    HBM, 'cam_matrix' on the host, already rescaled to (h, w) -- plus, in HBM, 'points' (n, 3) float32 (the dl-subsampled
    cloud), 'colors' (n, 3) float32, 'labels' (n,) int64 and 'pot_points' (np, 3) float32 (the caller's grid subsample at
    in_radius / 10, ScanNet_sphere_color.py:1039-1042). All scenes share (h, w). A scene without a point, a frame or a
    potential point is refused. init_potentials: a list of float64 arrays, default ``rand * 1e-3`` from the global NumPy
    generator like the reference (:330-334).

    The scenes are concatenated once (a copy: the list's own tensors can be dropped afterwards)."""

    def __init__(self, scene_dicts, in_radius, mask_margin=0.1, init_potentials=None):
        if not scene_dicts:
            raise ValueError("SphereScenes: at least one scene expected")
        frames = [SceneFrames(s) for s in scene_dicts]
        hw = {(f.h, f.w) for f in frames}
        if len(hw) != 1:
            raise ValueError("SphereScenes: every scene's frames must have the same (h, w), found %s" % sorted(hw))
        S = len(scene_dicts)
        points, colors, labels, pot_points = [], [], [], []
        table, pots = np.zeros((S, 8), np.int64), np.zeros((S, 2), np.int64)
        at = [0, 0, 0, 0, 0]
        for i, (s, f) in enumerate(zip(scene_dicts, frames)):
            p = _in_hbm("scene['points']", s['points'])
            c = _in_hbm("scene['colors']", s['colors'])
            lab = _in_hbm("scene['labels']", s['labels'])
            pp = _in_hbm("scene['pot_points']", s['pot_points'])
            if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != 3:
                raise RuntimeError("SphereScenes: points must be a float32 (num_points, 3) tensor")
            if c.dtype != torch.float32 or tuple(c.shape) != (p.shape[0], 3):
                raise RuntimeError("SphereScenes: colors must be a float32 (num_points, 3) tensor")
            if lab.dtype != torch.int64 or tuple(lab.shape) != (p.shape[0],):
                raise RuntimeError("SphereScenes: labels must be an int64 (num_points,) tensor")
            if pp.dtype != torch.float32 or pp.dim() != 2 or pp.shape[1] != 3:
                raise RuntimeError("SphereScenes: pot_points must be a float32 (num_pot, 3) tensor")
            if p.shape[0] < 1 or f.num_frames < 1:
                raise ValueError("SphereScenes: scene %d has no point or no frame" % i)
            if pp.shape[0] < 1:
                raise ValueError("SphereScenes: scene %d has no potential point" % i)
            points.append(p), colors.append(c), labels.append(lab), pot_points.append(pp)
            words = f.num_frames * ((f.num_base + 31) // 32)
            table[i] = (at[0], p.shape[0], at[1], f.num_base, at[2], f.num_frames, at[3], 0)
            pots[i] = (at[4], pp.shape[0])
            at = [at[0] + p.shape[0], at[1] + f.num_base, at[2] + f.num_frames, at[3] + words, at[4] + pp.shape[0]]
        device = points[0].device
        if init_potentials is None:
            init_potentials = [np.random.rand(int(n)) * 1e-3 for n in pots[:, 1]]
        if len(init_potentials) != S or any(len(p) != n for p, n in zip(init_potentials, pots[:, 1])):
            raise ValueError("SphereScenes: init_potentials must hold one value per potential point of every scene")
        potentials = torch.from_numpy(np.concatenate([np.asarray(p, np.float64) for p in init_potentials])).to(device)
        cam_inv = np.stack([f.cam_inv.reshape(9) for f in frames])
        self.resident = ops.TrainResident(
            torch.cat(points).contiguous(), torch.cat(labels).contiguous(),
            torch.cat([f.base_point_ind for f in frames]).contiguous(),
            torch.cat([f.overlap_bits.reshape(-1) for f in frames]).contiguous(),
            torch.cat([f.depth16 for f in frames]).contiguous(), torch.cat([f.images for f in frames]).contiguous(),
            torch.cat([f.poses for f in frames]).contiguous(), torch.from_numpy(cam_inv).to(device), table)
        self.sphere = ops.SphereResident(self.resident, torch.cat(colors).contiguous(), torch.cat(pot_points).contiguous(),
                                         potentials, pots)
        self.in_radius, self.mask_margin = float(in_radius), float(mask_margin)
        self.num_scenes, self.h, self.w = S, frames[0].h, frames[0].w

    def potentials(self, scene):
        """The current potentials of one scene: a view of the resident float64 buffer."""
        off, n = self.sphere.pots_host[scene].tolist()
        return self.sphere.potentials[off:off + n]


def draw_spheres(config, max_spheres, nv, flip=0.0):
    """The host's draws for max_spheres slots from the global NumPy generator, slot by slot in this order:
    ``rand(nv) < flip`` when flip is set; what ``augmentation_transform`` (datasets/common.py:259-302) draws except its
    ``randn`` -- ``rand()`` for 'vertical' or three ``rand()`` for 'all', ``rand(3)`` or ``rand()`` for the scale,
    ``randint(2, size=3)``; then ``rand()`` for ``augment_color``. Returns a list of dicts: 'flip' ([nv] bool or None),
    'rot', 'scale', 'sym', 'keep_color' (bool: the colours are kept unless rand() > augment_color)."""
    draws = []
    for _ in range(int(max_spheres)):
        d = {'flip': (np.random.rand(nv) < flip) if flip else None}
        d['rot'] = [np.random.rand() for _ in range({'vertical': 1, 'all': 3}.get(config.augment_rotation, 0))]
        d['scale'] = np.random.rand(3) if config.augment_scale_anisotropic else np.random.rand()
        d['sym'] = np.random.randint(2, size=3)
        d['keep_color'] = not (np.random.rand() > config.augment_color)
        draws.append(d)
    return draws


def augmentation_of(config, draw):
    """(R [3,3] float32, scale [3] float32) exactly as datasets/common.py:259-302 computes them from one slot's draws,
    including the isotropic form ``rand() * (max_s - min_s) - min_s`` as written there."""
    R = np.eye(3)
    if config.augment_rotation == 'vertical':
        theta = draw['rot'][0] * 2 * np.pi
        c, s = np.cos(theta), np.sin(theta)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    elif config.augment_rotation == 'all':
        theta = draw['rot'][0] * 2 * np.pi
        phi = (draw['rot'][1] - 0.5) * np.pi
        u = np.array([np.cos(theta) * np.cos(phi), np.sin(theta) * np.cos(phi), np.sin(phi)])
        alpha = draw['rot'][2] * 2 * np.pi
        R = create_3D_rotations(np.reshape(u, (1, -1)), np.reshape(alpha, (1, -1)))[0]
    R = R.astype(np.float32)
    min_s, max_s = config.augment_scale_min, config.augment_scale_max
    if config.augment_scale_anisotropic:
        scale = np.asarray(draw['scale'], np.float64) * (max_s - min_s) + min_s
    else:
        scale = float(draw['scale']) * (max_s - min_s) - min_s
    symmetries = np.array(config.augment_symmetries).astype(np.int32)
    symmetries = symmetries * np.asarray(draw['sym'], np.int32)
    return R, (scale * (1 - symmetries * 2)).astype(np.float32)


def stacked_3d_features(config, colors, world, use_point_color=False):
    """``stacked_3D_features`` of ScanNet_sphere_color.py:724-792 from colours [n,3] and the augmented points moved back
    by the centre [n,3] (column 2 is the height feature): a column of ones, then what the variant and its feature count
    ask for. Raises ValueError for an early-fusion count the reference does not know."""
    ones = torch.ones_like(world[:, :1])
    z, both = world[:, 2:], torch.cat([colors, world], 1)
    rgb_or_xyz = colors if use_point_color else world
    if getattr(config, 'late_fusion', False) or getattr(config, 'middle_fusion', False):
        dim = config.in_features_dim if getattr(config, 'late_fusion', False) else config.in_features_dim_3d
        extra = {2: z, 4: rgb_or_xyz, 7: both}.get(dim)
    elif getattr(config, 'early_fusion', False):
        table = {65: None, 66: z, 68: rgb_or_xyz, 69: torch.cat([colors, z], 1), 71: both}
        if config.in_features_dim not in table:
            raise ValueError('choose one fusion!')
        extra = table[config.in_features_dim]
    else:                                           # the baseline KPFCNN: the late-fusion table by its feature count
        extra = {2: z, 4: rgb_or_xyz, 7: both}.get(config.in_features_dim)
    return ones if extra is None else torch.cat([ones, extra], 1)


def sphere_batch(scenes, config, max_spheres, batch_limit, cap, num_rgbd_frames, k=3, flip=0.0, noise=None, draws=None,
                 use_point_color=False):
    """One batch of up to max_spheres spheres, picked by the resident potentials until they hold more than batch_limit
    points, as ``potential_item`` stacks it. A dict of HBM tensors; B_max = max_spheres, rows = cap:

    'points' (cap, 3) f32 centred and augmented, 'stack_lengths' (B_max,) int32, 'num_spheres' (1,) int32, 'cloud_inds' /
    'point_inds' (B_max,) int64 (-1 in a slot never reached), 'centers' (B_max, 3) f32, 'input_inds' (cap,) int64
    scene-local, 'labels' (cap,) int64, 'features' (cap, C) f32 (``stacked_3d_features``), 'feat_aggre_points' (cap, 3) f32,
    'images' (B_max, nv, 3, h, w) f32, 'image_xyz' (B_max, nv, h, w, 3) f32 (not augmented, as the reference), 'image_mask'
    (B_max, nv, h, w) bool, 'knn' (cap, k) int64 pixel numbers inside the sphere's views, 'knn_stacked' (cap, k) int64 (+ b *
    nv * h * w), 'scales' (B_max, 3) f32, 'rots' (B_max, 3, 3) f32, 'num_valid_pixels' (B_max,) int32, 'q_off' (B_max + 1,)
    int64 and 'status' (2,) int32: [0] rows dropped because they did not fit cap, [1] the same for the mask spheres (whose
    rows take at most 2 * cap). Rows at or past q_off[B_max] are zeros, -1 in the index outputs.

    scenes: a ``SphereScenes`` (its potentials are updated); config: augment_* and the variant's feature counts; flip:
    the probability of mirroring a view; noise: (cap, 3) f32 in HBM or None; draws: what ``draw_spheres`` returns (the
    default: drawn here). Everything goes up in one pinned upload; nothing is read back and nothing waits."""
    res, sres = scenes.resident, scenes.sphere
    B, nv, k, cap = int(max_spheres), int(num_rgbd_frames), int(k), int(cap)
    if B < 1 or cap < 1 or nv < 1:
        raise ValueError("sphere_batch: at least one slot, one row and one view expected")
    if draws is None:
        draws = draw_spheres(config, B, nv, flip)
    if len(draws) != B:
        raise ValueError("sphere_batch: one set of draws per slot expected")
    aug = [augmentation_of(config, d) for d in draws]
    big = np.finfo(np.float32).max
    # one upload of float32 words: R | scale | keep_color | the box no pixel leaves | flips as words
    flip_bytes = np.zeros(-(-B * nv // 4) * 4, np.uint8)
    has_flip = any(d.get('flip') is not None for d in draws)
    if has_flip:
        flip_bytes[:B * nv] = np.stack([np.zeros(nv, bool) if d.get('flip') is None else np.asarray(d['flip'], bool)
                                        for d in draws]).reshape(-1)
    words = np.concatenate([np.stack([a[0] for a in aug]).reshape(-1), np.stack([a[1] for a in aug]).reshape(-1),
                            np.array([1.0 if d['keep_color'] else 0.0 for d in draws], np.float32),
                            np.tile(np.array([-big, -big, big, big], np.float32), B),
                            flip_bytes.view(np.float32)]).astype(np.float32, copy=False)
    staged = torch.empty((len(words),), dtype=torch.float32, pin_memory=True)
    staged.numpy()[:] = words
    meta = staged.to(res.points.device, non_blocking=True)
    at = [0]

    def take(n):
        at[0] += n
        return meta[at[0] - n:at[0]]

    R_d, scale_d, keep_d, box_d = take(B * 9).view(B, 9), take(B * 3).view(B, 3), take(B), take(B * 4).view(B, 4)
    flips_d = take(len(flip_bytes) // 4).view(torch.uint8)[:B * nv].view(B, nv) if has_flip else None

    cloud_ind, point_ind, centers, _, num_spheres = ops.sphere_pick(sres, scenes.in_radius, batch_limit, B)
    status = torch.zeros((2,), device=cloud_ind.device, dtype=torch.int32)
    rows, q_off, _ = ops.sphere_members(res, cloud_ind, centers, scenes.in_radius, cap, status=status[0:1])
    mask_rows, mask_off, _ = ops.sphere_members(res, cloud_ind, centers, scenes.in_radius + scenes.mask_margin, 2 * cap,
                                                status=status[1:2])
    sel = ops.sphere_select_frames(res, cloud_ind, mask_rows, mask_off, nv)
    keys, image_xyz, image_mask, images, num_valid = ops.train_unproject(res, sel, cloud_ind, box_d, flips=flips_d)
    knn = ops.knn_f64_ragged(res.points, rows, q_off, keys, image_mask, k=k)
    r = ops.sphere_batch_rows(sres, cloud_ind, centers, rows, q_off, R_d, scale_d, keep_d, knn, nv * scenes.h * scenes.w,
                              noise=noise)
    return {'points': r['points'], 'stack_lengths': (q_off[1:] - q_off[:-1]).to(torch.int32), 'num_spheres': num_spheres,
            'cloud_inds': cloud_ind, 'point_inds': point_ind, 'centers': centers, 'input_inds': r['input_inds'],
            'labels': r['labels'], 'features': stacked_3d_features(config, r['colors'], r['world'], use_point_color),
            'feat_aggre_points': r['feat_aggre_points'], 'images': images, 'image_xyz': image_xyz, 'image_mask': image_mask,
            'knn': knn, 'knn_stacked': r['knn_stacked'], 'scales': scale_d, 'rots': R_d.view(B, 3, 3),
            'num_valid_pixels': num_valid, 'q_off': q_off, 'status': status, 'sel': sel}


def to_sphere_batch(out, config, limits=None, index_dtype=torch.int64, k=None):
    """The ``SphereBatch`` the networks take, from what ``sphere_batch`` returned: reads 'num_spheres', 'stack_lengths',
    'status' and 'num_valid_pixels' back in ONE copy -- the only wait of the path --, trims the rows and the slots to the
    spheres made, and builds the pyramid with ``segmentation_inputs_sphere(config, points, lengths, limits)``.

    Raises ValueError when 'status' reports rows that did not fit ``cap``, and -- in scikit-learn's words, as the
    reference's ball tree would -- when a sphere has fewer than k valid pixels."""
    B = out['cloud_inds'].shape[0]
    k = out['knn'].shape[1] if k is None else int(k)
    head = torch.cat([out['num_spheres'].to(torch.int32), out['status'], out['stack_lengths'], out['num_valid_pixels']])
    host = head.cpu().numpy()
    n, status, lens, valid = int(host[0]), host[1:3], host[3:3 + B], host[3 + B:3 + 2 * B]
    if status[0] or status[1]:
        raise ValueError("sphere_batch: the %s did not fit their capacity (cap = %d rows); raise cap"
                         % (" and the ".join(w for w, s in zip(("spheres", "mask spheres"), status) if s),
                            out['points'].shape[0]))
    lens = lens[:n].astype(np.int32)
    for b in range(n):
        if valid[b] < k:
            raise ValueError("Expected n_neighbors <= n_samples,  but n_samples = %d, n_neighbors = %d (sphere %d)"
                             % (valid[b], k, b))
    total = int(lens.sum())
    points, labels = out['points'][:total], out['labels'][:total]
    pyr = segmentation_inputs_sphere(config, points, lens, limits, index_dtype)
    if not any(getattr(config, a, False) for a in ('early_fusion', 'middle_fusion', 'late_fusion')):
        return SphereBatch(pyr, labels, features=out['features'][:total])
    offs = np.concatenate([[0], np.cumsum(lens)])
    batch = SphereBatch(pyr, labels, feature_3d=out['features'][:total],
                        feat_aggre_points=out['feat_aggre_points'][:total].unsqueeze(0), image_xyz=out['image_xyz'][:n],
                        images=out['images'][:n],
                        knn_list=[out['knn'][offs[b]:offs[b + 1]].unsqueeze(0) for b in range(n)])
    batch.knn_stacked = out['knn_stacked'][:total]
    return batch
