"""NumPy restatement of the sphere batches of the KPFCNN networks (reference: KPConv-PyTorch/datasets/
ScanNet_sphere_color.py:494-720 potential_item, :352-474 get_rgbd_data, datasets/common.py:252-316
augmentation_transform) with every random draw an argument, and of the ragged exact k-NN as a float64 lexsort on
(d2, index). The tests compare the device path (csrc/sphere_inputs.hip, dropin/datasets/sphere_inputs.py) with it bit for
bit; tests/test_sphere_inputs_cpu.py compares IT with what the reference's own functions produced (fixture g13)."""
import numpy as np


# ------------------------------------------------------------------------------------------------- the ragged k-NN

def sanitized_offsets(q_off, cap):
    """q_off as the library reads it: clamped to [0, cap] and made non-decreasing by a running maximum."""
    return np.maximum.accumulate(np.clip(np.asarray(q_off, np.int64), 0, cap))


def gather_queries(points, rows, q_off):
    """[cap,3] float32: points[rows[s]] in the slots of an item, zero where rows[s] lies outside [0, N) and in the slots
    of no item."""
    points, rows = np.asarray(points, np.float32), np.asarray(rows, np.int64)
    cap, lo = rows.shape[0], sanitized_offsets(q_off, rows.shape[0])
    out = np.zeros((cap, 3), np.float32)
    s = np.arange(cap)
    ok = (s >= lo[0]) & (s < lo[-1]) & (rows >= 0) & (rows < points.shape[0])
    out[ok] = points[rows[ok]]
    return out


def knn_one(queries, keys, valid, k, block=512):
    """[nq,k] int64: the k valid keys nearest to every query by (float64 d2, index), -1 where fewer exist. d2 is summed
    as the kernels sum it: ((dx*dx) + dy*dy) + dz*dz on float64 differences of the float32 queries."""
    q = np.asarray(queries, np.float32).astype(np.float64)
    keys = np.asarray(keys, np.float64)
    idx = np.nonzero(np.asarray(valid).astype(bool))[0] if valid is not None else np.arange(keys.shape[0])
    kk = keys[idx]
    out = np.full((q.shape[0], k), -1, np.int64)
    take = min(k, idx.shape[0])
    if take == 0:
        return out
    for a in range(0, q.shape[0], block):
        d = q[a:a + block, None, :] - kk[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.lexsort((np.broadcast_to(idx, d2.shape), d2), axis=1)[:, :take]      # by d2, then by index
        out[a:a + block, :take] = idx[order]
    return out


def knn_ragged(points, rows, q_off, keys, key_valid, k):
    """(knn [cap,k] int64, queries [cap,3] float32) of mvk_knn_f64_ragged."""
    rows = np.asarray(rows, np.int64)
    cap, lo = rows.shape[0], sanitized_offsets(q_off, rows.shape[0])
    queries = gather_queries(points, rows, q_off)
    knn = np.full((cap, k), -1, np.int64)
    for b in range(len(lo) - 1):
        if lo[b + 1] > lo[b]:
            knn[lo[b]:lo[b + 1]] = knn_one(queries[lo[b]:lo[b + 1]], keys[b], None if key_valid is None else key_valid[b], k)
    return knn, queries


# --------------------------------------------------------------------------------------------- spheres and potentials

def rdist(points32, center64):
    """sklearn's euclidean rdist of float32 points promoted to float64: ((dx*dx) + dy*dy) + dz*dz."""
    d = np.asarray(points32, np.float32).astype(np.float64) - np.asarray(center64, np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def tukey_update(pot_points32, potentials, center64, radius):
    """:571-581 in place: members by rdist <= r^2, weight (1 - sqrt(rdist)^2 / r^2)^2, zero where that square exceeds r^2."""
    r2 = float(radius) * float(radius)
    rd = rdist(pot_points32, center64)
    m = rd <= r2
    d2s = np.square(np.sqrt(rd[m]))
    t = np.square(1.0 - d2s / r2)
    t[d2s > r2] = 0.0
    potentials[m] += t


def pick(scenes, potentials, in_radius, batch_limit, max_spheres):
    """:556-602 with the stop rule :690-694. scenes: dicts with 'points' and 'pot_points' (float32); potentials: one float64
    array per scene, UPDATED in place. Returns the slots: dicts cloud_ind, point_ind, center (float32 [3]), input_inds
    (ascending, scene-local)."""
    mins = np.array([p.min() for p in potentials])
    args = np.array([int(p.argmin()) for p in potentials])
    slots, batch_n = [], 0
    while len(slots) < max_spheres:
        cloud = int(np.argmin(mins))                                   # the first among equals
        point = int(args[cloud])
        center = scenes[cloud]["pot_points"][point].astype(np.float32)
        tukey_update(scenes[cloud]["pot_points"], potentials[cloud], center.astype(np.float64), in_radius)
        args[cloud] = int(potentials[cloud].argmin())
        mins[cloud] = potentials[cloud][args[cloud]]
        inds = np.nonzero(rdist(scenes[cloud]["points"], center.astype(np.float64)) <= float(in_radius) * float(in_radius))[0]
        slots.append(dict(cloud_ind=cloud, point_ind=point, center=center, input_inds=inds.astype(np.int64)))
        batch_n += len(inds)
        if batch_n > int(batch_limit):
            break
    return slots


def members(points32, center32, radius):
    """The ascending scene-local numbers of the points with float64 rdist <= radius^2."""
    r = float(radius)
    return np.nonzero(rdist(points32, np.asarray(center32, np.float32).astype(np.float64)) <= r * r)[0].astype(np.int64)


# ------------------------------------------------------------------------------------------------------- augmentation

def rotation_all(theta, phi, alpha, create_3D_rotations):
    """datasets/common.py:270-283 given its three draws."""
    u = np.array([np.cos(theta) * np.cos(phi), np.sin(theta) * np.cos(phi), np.sin(phi)])
    return create_3D_rotations(np.reshape(u, (1, -1)), np.reshape(alpha, (1, -1)))[0]


def augment_params(config, draw, create_3D_rotations=None):
    """(R [3,3] float32, scale [3] float32) of datasets/common.py:259-302 from one slot's draws: draw['rot'] = the rand()
    values of the rotation (one for 'vertical', three for 'all', none otherwise), draw['scale'] = rand(3) or rand(),
    draw['sym'] = randint(2, size=3)."""
    R = np.eye(3)
    if config.augment_rotation == 'vertical':
        theta = draw['rot'][0] * 2 * np.pi
        c, s = np.cos(theta), np.sin(theta)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)
    elif config.augment_rotation == 'all':
        R = rotation_all(draw['rot'][0] * 2 * np.pi, (draw['rot'][1] - 0.5) * np.pi, draw['rot'][2] * 2 * np.pi,
                         create_3D_rotations)
    R = R.astype(np.float32)
    min_s, max_s = config.augment_scale_min, config.augment_scale_max
    if config.augment_scale_anisotropic:
        scale = np.asarray(draw['scale'], np.float64) * (max_s - min_s) + min_s
    else:
        scale = float(draw['scale']) * (max_s - min_s) - min_s        # as written there
    symmetries = np.array(config.augment_symmetries).astype(np.int32)
    symmetries = symmetries * np.asarray(draw['sym'], np.int32)
    scale = (scale * (1 - symmetries * 2)).astype(np.float32)
    return R, scale


def augment(x32, R, scale, noise):
    """datasets/common.py:316 in float32: ((x0 R0j + x1 R1j) + x2 R2j) * scale_j + noise_ij."""
    assert x32.dtype == np.float32 and R.dtype == np.float32 and scale.dtype == np.float32
    cols = [((x32[:, 0] * R[0, j] + x32[:, 1] * R[1, j]) + x32[:, 2] * R[2, j]) * scale[j] for j in range(3)]
    out = np.stack(cols, axis=1)
    return out + noise.astype(np.float32) if noise is not None else out


def features(config, colors, world, use_point_color=False):
    """stacked_3D_features of :724-792: ones, then the columns the variant and its feature count ask for.
    colors [n,3], world [n,3] float32 (the augmented points moved back by the centre; column 2 is the height)."""
    ones = np.ones((colors.shape[0], 1), np.float32)
    z, rgb_or_xyz, both = world[:, 2:], (colors if use_point_color else world), np.hstack([colors, world])
    late, middle, early = (getattr(config, a, False) for a in ("late_fusion", "middle_fusion", "early_fusion"))
    if late or middle:
        dim = config.in_features_dim if late else config.in_features_dim_3d
        extra = {1: None, 2: z, 4: rgb_or_xyz, 7: both}.get(dim, None)
        return ones if extra is None else np.hstack([ones, extra]).astype(np.float32)
    if early:
        table = {65: None, 66: z, 68: rgb_or_xyz, 69: np.hstack([colors, z]), 71: both}
        if config.in_features_dim not in table:
            raise ValueError('choose one fusion!')
        extra = table[config.in_features_dim]
        return ones if extra is None else np.hstack([ones, extra]).astype(np.float32)
    extra = {2: z, 4: rgb_or_xyz, 7: both}.get(config.in_features_dim, None)      # the baseline KPFCNN, by the same table
    return ones if extra is None else np.hstack([ones, extra]).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- views

def select_frames(overlap, base_point_ind, mask_inds, nv):
    """:361-376: the reference's greedy loop on the rows of the base points that lie in the mask sphere."""
    overlap = np.asarray(overlap).astype(bool)
    inside = np.isin(np.asarray(base_point_ind, np.int64), np.asarray(mask_inds, np.int64))
    rows, out = overlap[inside].copy(), []
    for _ in range(nv):
        f = int(rows.sum(0).argmax()) if rows.shape[0] else 0
        out.append(f)
        rows[rows[:, f]] = False
    return out


def unproject(cam_matrix, pose, depth_mm):
    """(xyz [h,w,3] float64 world, z_cam > 0 [h,w]) by the library's expression (csrc/unproject.h): the float32 inverse of
    the intrinsics widened, depth as float32 mm / 1000.f widened, ((k0*u + k1*v) + k2) * d, then ((c0*P0 + c1*P1) + c2*P2)
    + P3. The reference (:410-417) evaluates the same formula in another float order: see views()."""
    kinv = np.linalg.inv(np.asarray(cam_matrix, np.float32)[:3, :3]).astype(np.float64)
    d = (np.asarray(depth_mm).astype(np.uint16).astype(np.float32) / np.float32(1000.0)).astype(np.float64)
    v, u = np.indices(d.shape)
    u, v = u.astype(np.float64), v.astype(np.float64)
    c = [((kinv[r, 0] * u + kinv[r, 1] * v) + kinv[r, 2]) * d for r in range(3)]
    P = np.asarray(pose, np.float32).astype(np.float64)
    x = [((c[0] * P[r, 0] + c[1] * P[r, 1]) + c[2] * P[r, 2]) + P[r, 3] for r in range(3)]
    return np.stack(x, axis=-1), c[2] > 0.0


def views(scene, sel, flips=None):
    """The frames sel unprojected and mirrored where flips says so (:378-440): images (nv,h,w,3) float32, keys (nv*h*w,3)
    float64, image_mask (nv,h,w) -- depth > 0 alone: a sphere has no box."""
    images, xyz, masks = [], [], []
    for i, f in enumerate(sel):
        x, ok = unproject(scene["cam_matrix"], scene["poses"][f], scene["depth"][f])
        img = np.asarray(scene["images"][f], np.float32)
        if flips is not None and flips[i]:
            img, x, ok = np.fliplr(img), np.fliplr(x), np.fliplr(ok)
        images.append(img)
        xyz.append(x)
        masks.append(ok)
    return np.stack(images), np.stack(xyz).reshape(-1, 3), np.stack(masks)


# -------------------------------------------------------------------------------------------------------------- batch

def sphere_batch(scenes, potentials, config, max_spheres, batch_limit, nv, draws, k=3, mask_margin=0.1, noise=None,
                 use_point_color=False, create_3D_rotations=None):
    """potential_item (:494-720) with every draw given. scenes: host dicts with points, colors (float32), labels (int64),
    pot_points, base_point_ind, pointwise_rgbd_overlap, depth, images, poses, cam_matrix. draws[b]: dict with 'flip'
    ([nv] bool or None), 'rot', 'scale', 'sym' (augment_params) and 'keep_color' (bool: rand() <= augment_color).
    noise: [total,3] float32 rows in batch order, or None. potentials are updated in place. Rows inside a sphere are in
    ASCENDING point order. Returns the dict of dropin.datasets.sphere_inputs.sphere_batch, trimmed to the spheres."""
    slots = pick(scenes, potentials, config.in_radius, batch_limit, max_spheres)
    out = {key: [] for key in ("points", "world", "colors", "labels", "input_inds", "feat_aggre_points", "images",
                               "image_xyz", "image_mask", "knn", "knn_stacked", "scales", "rots", "sel", "keys")}
    at = 0
    for b, s in enumerate(slots):
        sc = scenes[s["cloud_ind"]]
        inds, c32 = s["input_inds"], s["center"]
        p = np.asarray(sc["points"], np.float32)[inds]
        mask_inds = members(sc["points"], c32, float(config.in_radius) + float(mask_margin))
        sel = select_frames(sc["pointwise_rgbd_overlap"], sc["base_point_ind"], mask_inds, nv)
        images, keys, mask = views(sc, sel, draws[b].get("flip"))
        knn = knn_one(p, keys, mask.reshape(-1), k)
        R, scale = augment_params(config, draws[b], create_3D_rotations)
        x = (p.astype(np.float64) - c32.astype(np.float64)).astype(np.float32)                         # :605
        aug = augment(x, R, scale, None if noise is None else noise[at:at + len(inds)])
        world = (aug.astype(np.float64) + c32.astype(np.float64)).astype(np.float32)                   # :664, :670
        colors = np.asarray(sc["colors"], np.float32)[inds] * np.float32(1.0 if draws[b]["keep_color"] else 0.0)
        npix = mask.size
        for key, v in (("points", aug), ("world", world), ("colors", colors), ("labels", np.asarray(sc["labels"], np.int64)[inds]),
                       ("input_inds", inds), ("feat_aggre_points", p), ("images", np.moveaxis(images, -1, 1)),
                       ("image_xyz", keys.astype(np.float32).reshape(mask.shape + (3,))), ("image_mask", mask),
                       ("knn", knn), ("knn_stacked", np.where(knn >= 0, knn + b * npix, -1)), ("scales", scale), ("rots", R),
                       ("sel", np.asarray(sel, np.int32)), ("keys", keys)):
            out[key].append(v)
        at += len(inds)
    cat = {key: np.concatenate(out[key], 0) for key in ("points", "world", "colors", "labels", "input_inds",
                                                        "feat_aggre_points", "knn", "knn_stacked")}
    stk = {key: np.stack(out[key], 0) for key in ("images", "image_xyz", "image_mask", "scales", "rots", "sel", "keys")}
    res = dict(cat, **stk)
    res.update(stack_lengths=np.array([len(s["input_inds"]) for s in slots], np.int32),
               cloud_inds=np.array([s["cloud_ind"] for s in slots], np.int64),
               point_inds=np.array([s["point_ind"] for s in slots], np.int64),
               centers=np.stack([s["center"] for s in slots]), num_spheres=len(slots),
               features=features(config, cat["colors"], cat["world"], use_point_color))
    return res


# -------------------------------------------------------------------------------------------------------------- scenes

def synthetic_scene(seed, n, nf=12, nb=200, h=12, w=16, ext=(3.0, 2.5, 2.0), pot_dl=0.3):
    """A host scene dict: n points in a box with colours and labels, coarse potential points (a grid subsample's stand-in:
    one point per occupied cell of pot_dl, the cell's first point), base points with an overlap table, and frames looking
    along +z from below the scene, each shifted in xy; frame 1 has no valid depth, frame 2 has holes."""
    rng = np.random.default_rng(seed)
    points = (rng.random((n, 3)) * np.asarray(ext) + np.asarray([0.1, 0.3, 0.0])).astype(np.float32)
    cells = np.floor(points / np.float32(pot_dl)).astype(np.int64)
    _, first = np.unique(cells, axis=0, return_index=True)
    cam = np.array([[6.0, 0, w / 2], [0, 6.0, h / 2], [0, 0, 1]], np.float32)
    depth = rng.integers(900, 2100, size=(nf, h, w)).astype(np.uint16)
    depth[1] = 0
    depth[2][rng.random((h, w)) < 0.3] = 0
    poses = np.tile(np.eye(4, dtype=np.float32), (nf, 1, 1))
    centre = (points.max(0) + points.min(0)) / 2
    for f in range(nf):
        poses[f, :3, 3] = (centre[0] + 0.25 * (f - nf / 2), centre[1] - 0.2 * (f - nf / 2), -1.0)
    return {"points": points, "colors": rng.random((n, 3)).astype(np.float32), "labels": rng.integers(0, 20, n).astype(np.int64),
            "pot_points": points[np.sort(first)].copy(), "depth": depth,
            "images": rng.standard_normal((nf, h, w, 3)).astype(np.float32), "poses": poses, "cam_matrix": cam,
            "base_point_ind": np.sort(rng.choice(n, nb, replace=False)).astype(np.int64),
            "pointwise_rgbd_overlap": rng.random((nb, nf)) < 0.3}


# ----------------------------------------------------------------------------------------------------- fixture g18

class _Config(object):
    pass


def golden_case(g, name):
    """One case of tests/golden/g18_sphere_batch.npz (written by tests/golden/make_g18_sphere_batch.py from the
    reference's own potential_item): the scenes and initial potentials, the config, the logged draws as draw dicts, and
    the case's arrays under their fixture names."""
    S = int(g["num_scenes"])
    scenes = [{key: g["scene%d/%s" % (i, key)] for key in ("points", "colors", "labels", "pot_points", "base_point_ind",
                                                           "pointwise_rgbd_overlap", "depth", "images", "poses", "cam_matrix")}
              for i in range(S)]
    cfg = _Config()
    cfg.in_radius = float(g["in_radius"])
    cfg.augment_rotation = str(g["augment_rotation"])
    cfg.augment_scale_anisotropic = bool(g["augment_scale_anisotropic"])
    cfg.augment_scale_min, cfg.augment_scale_max = float(g["augment_scale_min"]), float(g["augment_scale_max"])
    cfg.augment_symmetries = [bool(v) for v in g["augment_symmetries"]]
    cfg.augment_color, cfg.augment_noise = float(g["augment_color"]), float(g["augment_noise"])
    cfg.early_fusion, cfg.in_features_dim = True, int(g["in_features_dim"])
    case = {key[len(name) + 1:]: g[key] for key in g.files if key.startswith(name + "/")}
    n = len(case["stack_lengths"])
    draws = [dict(flip=case["flip_rand"][b] < float(g["flip"]), rot=case["rot_rand"][b], scale=case["scale_rand"][b],
                  sym=case["sym_rand"][b], keep_color=not (case["color_rand"][b] > cfg.augment_color)) for b in range(n)]
    case.update(scenes=scenes, potentials=[g["potentials%d" % i] for i in range(S)], config=cfg, draws=draws,
                max_spheres=n, nv=int(g["nv"]), k=int(g["k"]), mask_margin=0.1)
    return case


def golden_order(g):
    """Per sphere, the permutation that puts the reference's rows (its KD-tree's order) into ascending input_inds."""
    offs = np.concatenate([[0], np.cumsum(g["stack_lengths"])])
    return np.concatenate([offs[b] + np.argsort(g["input_inds"][offs[b]:offs[b + 1]], kind="stable")
                           for b in range(len(offs) - 1)])


def golden_noise_rows(g, cap=None):
    """The reference's noise rows, put where the ascending row order adds them; zero rows up to cap."""
    noise = g["noise"][golden_order(g)]
    if cap is None:
        return noise
    out = np.zeros((cap, 3), np.float32)
    out[:len(noise)] = noise
    return out


def compare_with_golden(out, g):
    """out: the dict of sphere_batch (here or on the device) as host arrays. The index ORDER inside a sphere is ascending
    here and the tree's there: the reference's rows are sorted by input_inds before they are compared. Exact: points,
    features, labels, input_inds, cloud_inds, point_inds, stack_lengths, images, image_mask, knn, scales, rots,
    feat_aggre_points. Returns the largest image_xyz difference in float32 ulp of the largest coordinate."""
    n, total = len(g["stack_lengths"]), int(g["stack_lengths"].sum())
    assert int(np.asarray(out["num_spheres"]).reshape(-1)[0]) == n
    order = golden_order(g)

    def eq(a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what

    eq(np.asarray(out["stack_lengths"])[:n], g["stack_lengths"], "stack_lengths")
    eq(np.asarray(out["cloud_inds"])[:n].astype(np.int32), g["cloud_inds"], "cloud_inds")
    eq(np.asarray(out["point_inds"])[:n].astype(np.int32), g["point_inds"], "point_inds")
    for key, theirs in (("points", "stacked_points"), ("features", "features"), ("labels", "labels"),
                        ("input_inds", "input_inds"), ("knn", "knn"), ("feat_aggre_points", "feat_aggre_points")):
        eq(np.asarray(out[key])[:total], g[theirs][order], key)
    eq(np.asarray(out["images"])[:n], g["images"], "images")
    eq(np.asarray(out["image_mask"])[:n].astype(bool), g["image_mask"], "image_mask")
    eq(np.asarray(out["scales"])[:n], g["scales"], "scales")
    eq(np.asarray(out["rots"])[:n].reshape(n, 3, 3), g["rots"], "rots")
    mine, theirs = np.asarray(out["image_xyz"])[:n].astype(np.float64), g["image_xyz"].astype(np.float64)
    return float(np.abs(mine - theirs).max() / np.spacing(np.float32(np.abs(theirs).max())))
