"""NumPy restatements for the tests of csrc/train_inputs.hip (training batches of the MVPNet baseline from resident
scenes): ScanNet2D3DChunks.__getitem__ and get_rgbd_data (mvpnet/data/scannet_2d3d.py:323-416, :191-321) with every draw
an argument -- the candidate centres, the resample's choice, the flip flags, the rotation -- plus the library's own
resample rule (mix32 / draw / key in uint32 and uint64 arithmetic) and the synthetic scenes the tests share. Nothing here
reads the reference tree.

The crop is float32 comparisons, the frame choice integer arithmetic (tests/scene_inputs_ref.py), the unprojection
csrc/unproject.h's float64 expression in its order, the mask a strict float64 comparison against (double)box -+ 0.1 (the
NumPy 1.x reading of :274-281), the k-NN a brute-force float64 search (ties: the lower pixel), the rotation
m[r][0]*x + m[r][1]*y + m[r][2]*z in float64, left to right, on the float32 values."""
import numpy as np

import scene_inputs_ref as sref

PIXEL_MARGIN = 0.1
IGNORE_LABEL = -100
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------ resample rule

def mix32(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, mod 2^32 (uint64 arrays in, out)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def draw(seed, i):
    """draw(i) = mix32(lo32(seed) ^ mix32(hi32(seed) + i * 0x9e3779b9)) for an int64 seed and positions i."""
    s = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    lo, hi = s & M32, s >> np.uint64(32)
    i = np.asarray(i, dtype=np.uint64) & M32
    return mix32(lo ^ mix32((hi + ((i * np.uint64(0x9e3779b9)) & M32)) & M32))


def keys_of(seed, n, key_bits=32):
    return draw(seed, np.arange(n)) >> np.uint64(32 - key_bits)


def resample_positions(nc, nb_pts, seed, key_bits=32):
    """[nb_pts] int64 positions of a row of nc entries: the nb_pts first in (key, position) order, ascending, when
    nc >= nb_pts; else 0 .. nc-1 and the pads (uint64(draw(nc + j)) * nc) >> 32; -1 of an empty row."""
    if nc == 0:
        return np.full(nb_pts, -1, np.int64)
    if nc >= nb_pts:
        order = np.lexsort((np.arange(nc), keys_of(seed, nc, key_bits)))           # by key, then by position
        return np.sort(order[:nb_pts]).astype(np.int64)
    pad = (draw(seed, nc + np.arange(nb_pts - nc)) * np.uint64(nc)) >> np.uint64(32)
    return np.concatenate([np.arange(nc), pad.astype(np.int64)]).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------- the crop

def crop(points, seg_label, centers, chunk_size=(1.5, 1.5), chunk_margin=(0.2, 0.2), chunk_thresh=0.3):
    """:340-371 with the centres given: (counts [T,2] int32 of every try, chosen, box [4] f32 (lo.x, lo.y, hi.x, hi.y),
    chunk_mask [n] bool). A centre outside the scene counts nothing."""
    size, margin = np.asarray(chunk_size, np.float32), np.asarray(chunk_margin, np.float32)
    xy = points[:, :2]
    counts = np.zeros((len(centers), 2), np.int32)
    chosen, best = -1, None
    for t, c in enumerate(np.asarray(centers).tolist()):
        if not 0 <= c < len(points):
            continue
        center = points[c][:2]
        lo = (center - np.float32(0.5) * size) - margin
        hi = (center + np.float32(0.5) * size) + margin
        assert lo.dtype == np.float32 and hi.dtype == np.float32
        mask = np.all(np.logical_and(xy >= lo, xy <= hi), axis=1)
        labeled = seg_label[mask] >= 0
        counts[t] = (mask.sum(), labeled.sum())
        if chosen < 0 and len(labeled) > 0 and np.mean(labeled) >= chunk_thresh:
            chosen, best = t, (lo, hi, mask)
    if chosen < 0:
        best = (np.min(xy, axis=0) - margin, np.max(xy, axis=0) + margin, np.ones(len(points), bool))
    lo, hi, mask = best
    return counts, chosen, np.hstack([lo, hi]).astype(np.float32), mask


# ------------------------------------------------------------------------------------------------------------- frames

def unproject(cam_matrix, pose, depth_mm):
    """(xyz [h,w,3] f64 world, z_cam > 0 [h,w]) by csrc/unproject.h: the float32 inverse of the intrinsics widened, depth
    as float32 mm / 1000.f widened, ((k0*u + k1*v) + k2) * d, then ((c0*P0 + c1*P1) + c2*P2) + P3."""
    kinv = np.linalg.inv(np.asarray(cam_matrix, np.float32)[:3, :3]).astype(np.float64)
    d = (np.asarray(depth_mm).astype(np.uint16).astype(np.float32) / np.float32(1000.0)).astype(np.float64)
    v, u = np.indices(d.shape)
    u, v = u.astype(np.float64), v.astype(np.float64)
    c = [((kinv[r, 0] * u + kinv[r, 1] * v) + kinv[r, 2]) * d for r in range(3)]
    P = np.asarray(pose, np.float32).astype(np.float64)
    x = [((c[0] * P[r, 0] + c[1] * P[r, 1]) + c[2] * P[r, 2]) + P[r, 3] for r in range(3)]
    return np.stack(x, axis=-1), c[2] > 0.0


def box_bounds(box):
    """(xlo, xhi, ylo, yhi) float64 of a float32 (lo.x, lo.y, hi.x, hi.y): (double)box -+ 0.1."""
    b = np.asarray(box, np.float32).astype(np.float64)
    return np.array([b[0] - PIXEL_MARGIN, b[2] + PIXEL_MARGIN, b[1] - PIXEL_MARGIN, b[3] + PIXEL_MARGIN], np.float64)


def rotate(m, xyz32):
    """m [3,3] f64, xyz32 (..., 3) f32 -> f32: m[r][0]*x + m[r][1]*y + m[r][2]*z in float64, left to right."""
    assert xyz32.dtype == np.float32
    x, y, z = (xyz32[..., a].astype(np.float64) for a in range(3))
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z).astype(np.float32) for r in range(3)], axis=-1)


def knn(queries32, keys64, valid, k):
    """[nq,k] int64: the k valid keys nearest to each float32 query in float64, (dx*dx + dy*dy) + dz*dz, ascending by
    (distance, index); -1 where fewer than k keys are valid."""
    ind = np.nonzero(valid)[0]
    q = queries32.astype(np.float64)
    out = np.full((len(q), k), -1, np.int64)
    if len(ind) == 0:
        return out
    kk = keys64[ind]
    dx, dy, dz = (q[:, None, a] - kk[None, :, a] for a in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]                # stable: the lower index among equals
    out[:, :order.shape[1]] = ind[order]
    return out


def rgbd(scene, chunk_row, box, sample_points, nv, k, flips=None):
    """:191-321 for one chunk: chunk_row = the scene-local, ascending point numbers of the chunk BEFORE the resample,
    sample_points [nb_pts,3] f32 after it. Returns sel, images (nv,h,w,3), keys (nv*h*w,3) f64, image_mask (nv,h,w)."""
    sel = sref.select_frames_of_chunk(scene["pointwise_rgbd_overlap"], scene["base_point_ind"], chunk_row, nv)
    images, keys, mask = views(scene, sel, box, flips)
    return sel, images, keys, mask, knn(sample_points, keys, mask.reshape(-1), k)


def views(scene, sel, box, flips=None):
    """The frames sel of a scene unprojected, masked by the box and mirrored where flips says so: images (nv,h,w,3),
    keys (nv*h*w,3) f64, image_mask (nv,h,w)."""
    bounds = box_bounds(box)
    images, xyz, masks = [], [], []
    for i, f in enumerate(sel):
        x, ok = unproject(scene["cam_matrix"], scene["poses"][f], scene["depth"][f])
        m = sref.pixel_mask(x, ok, bounds)
        img = scene["images"][f]
        if flips is not None and flips[i]:
            img, x, m = np.fliplr(img), np.fliplr(x), np.fliplr(m)
        images.append(img)
        xyz.append(x)
        masks.append(m)
    return np.stack(images), np.stack(xyz).reshape(-1, 3), np.stack(masks)


def item(scene, centers, nb_pts, nv, k=3, seed=0, choice=None, flips=None, rot=None, chunk_size=(1.5, 1.5),
         chunk_thresh=0.3, chunk_margin=(0.2, 0.2), key_bits=32):
    """__getitem__ (to_tensor=True) with the draws given. choice: the resample's positions in the chunk (the reference's
    crop_pad_choice), or None for the library's rule with `seed`. rot: the [3,3] float64 rotation or None."""
    points, seg_label = scene["points"], scene["seg_label"]
    counts, chosen, box, mask = crop(points, seg_label, centers, chunk_size, chunk_margin, chunk_thresh)
    row = np.nonzero(mask)[0]
    pos = resample_positions(len(row), nb_pts, seed, key_bits) if choice is None else np.asarray(choice, np.int64)
    sample = row[pos]
    pts, lab = points[sample], seg_label[sample]
    sel, images, keys, image_mask, knn_indices = rgbd(scene, row, box, pts, nv, k, flips)
    image_xyz = keys.astype(np.float32).reshape(image_mask.shape + (3,))
    if rot is not None:
        pts, image_xyz = rotate(rot, pts), rotate(rot, image_xyz)
    return {"points": np.ascontiguousarray(pts.T), "seg_label": lab, "images": np.ascontiguousarray(np.moveaxis(images, -1, 1)),
            "image_xyz": image_xyz, "image_mask": image_mask, "knn_indices": knn_indices, "chunk_try": chosen,
            "num_valid_pixels": int(image_mask.sum()), "counts": counts, "box": box, "row": row, "positions": pos,
            "sel": sel, "keys": keys}


# ------------------------------------------------------------------------------------------------------------- scenes

def synthetic_scene(seed, n, nf=5, nb=400, h=12, w=16, ext=(3.0, 2.5, 2.0), unlabeled=0.3):
    """A host scene dict: n points in a box, training labels with a share of -100, and scene_inputs_ref's frames."""
    rng = np.random.default_rng(seed)
    points = (rng.random((n, 3)) * np.asarray(ext) + np.asarray([0.1, 0.3, 0.0])).astype(np.float32)
    seg_label = rng.integers(0, 20, n).astype(np.int64)
    seg_label[rng.random(n) < unlabeled] = IGNORE_LABEL
    scene = sref.synthetic_frames(points, nf=nf, h=h, w=w, nb=nb, seed=seed + 100)
    scene.update(points=points, seg_label=seg_label)
    return scene
