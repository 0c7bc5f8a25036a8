#!/usr/bin/env python3
"""Generate tests/golden/g18_sphere_batch.npz from the REFERENCE ITSELF (build container, CPU only).

Run from the repo root:   python tests/golden/make_g18_sphere_batch.py

The reference's ScanNetDataset (KPConv-PyTorch/datasets/ScanNet_sphere_color.py) is imported from the reference tree at
generation time and its OWN potential_item, get_rgbd_data and augmentation_transform are executed -- called as unbound
functions on a light stand-in object that carries the attributes they read: scikit-learn KDTrees of the potential points
and of the input clouds (leaf_size 10, as load_subsampled_clouds builds them), the potentials as torch tensors, the
sub_rgbd_dict, a config, and a segmentation_inputs_sphere that returns its arguments. The frames are PNG / text files in
a temporary directory. Modules the reference imports but this container lacks (open3d, torchvision, natsort, plyfile,
its compiled wrappers) are stubbed in sys.modules: none of them is reached. np.random's rand / randint / randn are wrapped
so that every value the reference draws is logged; get_rgbd_data is wrapped so that its image_mask, which potential_item
drops, is kept.

Two scenes of tests/sphere_inputs_ref.synthetic_scene (<= 3 000 points, 12 frames of 12 x 16, 200 base points), nv = 3,
k = 3, in_radius 0.8, 'vertical' rotation, anisotropic scale, a symmetry in x, flip 0.5, augment_color 0.7, early
fusion with in_features_dim 66. Two cases from the same initial potentials:

  stop2   batch_limit reached with the second sphere
  stop3   batch_limit reached with the third sphere

Per case, only arrays: the draws (flip_rand [n,nv], rot_rand [n,1], scale_rand [n,3], sym_rand [n,3], color_rand [n], noise
[total,3] float32 in the reference's row order) and the outputs (stacked_points, features, labels, input_inds, cloud_inds,
point_inds, stack_lengths, feat_aggre_points, images, image_xyz, image_mask, knn, scales, rots, potentials_after<i>).

The generator re-draws its seed until the conditions hold that make an exact comparison fair -- checked on the
reference's own values: no point and no potential point within 1e-9 (relative) of an r^2 bound (in_radius for both,
in_radius + 0.1 for the points); the k + 1 nearest distances of every query distinct by more than 1e-9; no two scene
minima of the potentials equal at any pick -- and until the case shows what it is for: a flipped and an unflipped view,
a sphere with the symmetry applied and one without, a colour drop and a kept colour. Before writing, it checks that the
restatement (tests/sphere_inputs_ref.py) fed the logged draws reproduces every exact output.

Only DATA is written; no reference source text."""
import contextlib
import functools
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g18_sphere_batch.npz")
REFROOT = "/root/reference/KPConv-PyTorch"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sphere_inputs_ref as ref  # noqa: E402

NV, K, H, W, NF, NB = 3, 3, 12, 16, 12, 200
IN_RADIUS, FLIP = 0.8, 0.5
SIZES = (2600, 3000)


class _Anything(types.ModuleType):
    """A stand-in for a module this container lacks: any attribute is another stand-in, callable."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        child = _Anything(self.__name__ + "." + name)
        setattr(self, name, child)
        return child

    def __call__(self, *a, **kw):
        return self


def stub_missing(names):
    for name in names:
        try:
            __import__(name)
        except ImportError:
            parts = name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), _Anything(".".join(parts[:i])))


class DrawLog(object):
    """Wraps np.random.rand / randint / randn and keeps what they returned."""

    def __init__(self):
        self.calls, self.saved = [], {}

    def __enter__(self):
        for name in ("rand", "randint", "randn"):
            self.saved[name] = getattr(np.random, name)

            def wrapped(*a, _name=name, **kw):
                out = self.saved[_name](*a, **kw)
                self.calls.append((_name, a, kw, np.copy(out)))
                return out
            setattr(np.random, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(np.random, name, fn)


def write_frames(tmp, scan_id, scene):
    from PIL import Image
    d = os.path.join(tmp, scan_id)
    for sub in ("color", "depth", "pose"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    frame_ids = [str(100 + 7 * f) for f in range(NF)]
    for f, fid in enumerate(frame_ids):
        Image.fromarray(scene["color_u8"][f]).save(os.path.join(d, "color", fid + ".png"))
        Image.fromarray(scene["depth"][f].astype(np.uint16)).save(os.path.join(d, "depth", fid + ".png"))
        np.savetxt(os.path.join(d, "pose", fid + ".txt"), scene["poses"][f], fmt="%.9g")
    return frame_ids


def make_scenes():
    scenes = []
    for i, n in enumerate(SIZES):
        s = ref.synthetic_scene(180 + i, n, nf=NF, nb=NB, h=H, w=W)
        s["color_u8"] = np.random.default_rng(280 + i).integers(0, 256, size=(NF, H, W, 3)).astype(np.uint8)
        s["images"] = s["color_u8"].astype(np.float32) / 255.             # what the reference reads back (:401)
        scenes.append(s)
    return scenes


def standin(mod, common, torch, scenes, potentials, tmp, frame_ids, batch_limit, masks):
    from sklearn.neighbors import KDTree
    cfg = types.SimpleNamespace(in_radius=IN_RADIUS, augment_rotation='vertical', augment_scale_anisotropic=True,
                                augment_scale_min=0.9, augment_scale_max=1.1, augment_symmetries=[True, False, False],
                                augment_noise=0.005, augment_color=0.7, late_fusion=False, middle_fusion=False,
                                early_fusion=True, in_features_dim=66)
    me = types.SimpleNamespace(
        config=cfg, set='training', image_dir=tmp, resize=None, resize_scale=None, color_jitter=None, image_normalizer=None,
        flip=FLIP, k=K, num_rgbd_frames=NV, use_point_color=False, batch_limit=batch_limit, worker_lock=contextlib.nullcontext(),
        cloud_names=["scene%04d_00" % i for i in range(len(scenes))],
        sub_rgbd_dict=[{"scan_id": "scene%04d_00" % i, "sub_base_point_ind": s["base_point_ind"].astype(np.int32),
                        "sub_pointwise_rgbd_overlap": s["pointwise_rgbd_overlap"], "frame_ids": frame_ids[i],
                        "cam_matrix": s["cam_matrix"].astype(np.float64)} for i, s in enumerate(scenes)],
        pot_trees=[KDTree(s["pot_points"], leaf_size=10) for s in scenes],
        input_trees=[KDTree(s["points"], leaf_size=10) for s in scenes],
        input_colors=[s["colors"] for s in scenes], input_labels=[s["labels"] for s in scenes],
        potentials=[torch.from_numpy(p.copy()) for p in potentials],
        segmentation_inputs_sphere=lambda *a: list(a))
    mins = [torch.min(p, 0) for p in me.potentials]
    me.min_potentials = torch.stack([m.values for m in mins])
    me.argmin_potentials = torch.stack([m.indices for m in mins])
    me._get_paths = functools.partial(mod.ScanNetDataset._get_paths, me)
    me.augmentation_transform = functools.partial(common.PointCloudDataset.augmentation_transform, me)

    def get_rgbd_data(*a):
        out = mod.ScanNetDataset.get_rgbd_data(me, *a)
        masks.append(out[3][0])
        return out
    me.get_rgbd_data = get_rgbd_data
    return me


def parse_draws(calls, lengths):
    """The log in the reference's order per sphere: nv flips, theta, scale, symmetries, noise, colour."""
    calls = list(calls)
    out = dict(flip_rand=[], rot_rand=[], scale_rand=[], sym_rand=[], color_rand=[], noise=[])
    for n in lengths:
        flips = []
        for _ in range(NV):
            name, a, _, v = calls.pop(0)
            assert name == "rand" and a == ()
            flips.append(float(v))
        name, a, _, theta = calls.pop(0)
        assert name == "rand" and a == ()
        name, a, _, scale = calls.pop(0)
        assert name == "rand" and a == (3,)
        name, a, kw, sym = calls.pop(0)
        assert name == "randint" and a == (2,) and kw == {"size": 3}
        name, a, _, normal = calls.pop(0)
        assert name == "randn" and a == (n, 3)
        name, a, _, col = calls.pop(0)
        assert name == "rand" and a == ()
        out["flip_rand"].append(flips), out["rot_rand"].append([float(theta)]), out["scale_rand"].append(scale)
        out["sym_rand"].append(sym), out["color_rand"].append(float(col))
        out["noise"].append((normal * 0.005).astype(np.float32))
    assert not calls
    return dict(flip_rand=np.array(out["flip_rand"]), rot_rand=np.array(out["rot_rand"]), scale_rand=np.array(out["scale_rand"]),
                sym_rand=np.array(out["sym_rand"], np.int64), color_rand=np.array(out["color_rand"]),
                noise=np.concatenate(out["noise"], 0))


def near(values, bound, rel=1e-9):
    return np.abs(np.asarray(values) - bound).min() <= rel * bound


def fair(scenes, potentials, case, masks, n_spheres):
    """The conditions of an exact comparison, on the reference's values and the restatement's replay of its picks."""
    pots = [p.copy() for p in potentials]
    mins = np.array([p.min() for p in pots])
    offs = np.concatenate([[0], np.cumsum(case["stack_lengths"])])
    for b in range(n_spheres):
        if len(np.unique(mins)) != len(mins):
            return "two scene minima of the potentials equal"
        s = scenes[case["cloud_inds"][b]]
        c = s["pot_points"][case["point_inds"][b]].astype(np.float64)
        if near(ref.rdist(s["pot_points"], c), IN_RADIUS ** 2) or near(ref.rdist(s["points"], c), IN_RADIUS ** 2) \
                or near(ref.rdist(s["points"], c), (IN_RADIUS + 0.1) ** 2):
            return "a point within 1e-9 of an r^2 bound"
        ref.tukey_update(s["pot_points"], pots[case["cloud_inds"][b]], c, IN_RADIUS)
        mins[case["cloud_inds"][b]] = pots[case["cloud_inds"][b]].min()
        valid = masks[b].reshape(-1)
        if valid.sum() < K + 1:
            return "fewer than k + 1 valid pixels"
        q = case["feat_aggre_points"][offs[b]:offs[b + 1]].astype(np.float64)
        kk = case["image_xyz64"][b].reshape(-1, 3)[valid]
        d = np.sqrt(((q[:, None, :] - kk[None, :, :]) ** 2).sum(-1))
        d.sort(axis=1)
        if np.diff(d[:, :K + 1], axis=1).min() <= 1e-9:
            return "two of the k + 1 nearest distances within 1e-9"
    return None


def header(scenes, potentials):
    out = dict(num_scenes=np.array(len(scenes)), in_radius=np.array(IN_RADIUS), augment_rotation=np.array('vertical'),
               augment_scale_anisotropic=np.array(True), augment_scale_min=np.array(0.9), augment_scale_max=np.array(1.1),
               augment_symmetries=np.array([True, False, False]), augment_color=np.array(0.7), augment_noise=np.array(0.005),
               in_features_dim=np.array(66), flip=np.array(FLIP), nv=np.array(NV), k=np.array(K))
    for i, s in enumerate(scenes):
        for key in ("points", "colors", "labels", "pot_points", "base_point_ind", "pointwise_rgbd_overlap", "depth", "images",
                    "poses", "cam_matrix"):
            out["scene%d/%s" % (i, key)] = s[key]
        out["potentials%d" % i] = potentials[i]
    return out


class _Npz(dict):
    files = property(lambda self: list(self))


def run_case(mod, common, torch, name, scenes, n_spheres, potentials, seed):
    """The reference on the scenes from the given potentials with np.random seeded by `seed`, the batch limit set so that
    the batch stops with sphere n_spheres. Returns the case's arrays; LookupError when the seed does not serve."""
    sizes = [len(s["input_inds"]) for s in ref.pick(scenes, [p.copy() for p in potentials], IN_RADIUS, 1 << 40, n_spheres)]
    batch_limit = int(np.sum(sizes)) - 1
    masks = []
    with tempfile.TemporaryDirectory() as tmp:
        frame_ids = [write_frames(tmp, "scene%04d_00" % i, s) for i, s in enumerate(scenes)]
        me = standin(mod, common, torch, scenes, potentials, tmp, frame_ids, batch_limit, masks)
        np.random.seed(seed)
        with DrawLog() as log:
            out = mod.ScanNetDataset.potential_item(me, 0)
    (stacked_points, image_xyz, images, feat_aggre_points, labels, stack_lengths, scales, rots, cloud_inds, point_inds,
     input_inds, knn_list, features) = out
    if len(stack_lengths) != n_spheres:
        raise LookupError("the batch stopped elsewhere")
    draws = parse_draws(log.calls, stack_lengths)
    flips = draws["flip_rand"] < FLIP
    keep = ~(draws["color_rand"] > 0.7)
    if flips.all() or not flips.any() or draws["sym_rand"][:, 0].all() or not draws["sym_rand"][:, 0].any() \
            or keep.all() or not keep.any():
        raise LookupError("the draws do not show every branch")
    case = dict(draws, stacked_points=stacked_points, features=features, labels=labels.astype(np.int64),
                input_inds=input_inds.astype(np.int64), cloud_inds=cloud_inds, point_inds=point_inds,
                stack_lengths=stack_lengths, feat_aggre_points=feat_aggre_points[0], images=images, image_xyz=image_xyz,
                image_mask=np.stack(masks), knn=np.concatenate([k[0] for k in knn_list], 0), scales=scales, rots=rots,
                batch_limit=np.array(batch_limit))
    case["image_xyz64"] = np.stack([
        ref.views(scenes[c], ref.select_frames(scenes[c]["pointwise_rgbd_overlap"], scenes[c]["base_point_ind"],
                                               ref.members(scenes[c]["points"], scenes[c]["pot_points"][p], IN_RADIUS + 0.1), NV),
                  flips[b])[1] for b, (c, p) in enumerate(zip(cloud_inds, point_inds))])
    why = fair(scenes, potentials, case, masks, n_spheres)
    if why:
        print("  %s seed %d: %s" % (name, seed, why))
        raise LookupError(why)
    del case["image_xyz64"]
    for i, p in enumerate(me.potentials):
        case["potentials_after%d" % i] = p.numpy().copy()
    return case


def find_case(mod, common, torch, name, scenes, n_spheres, potentials):
    for seed in range(200):
        try:
            return run_case(mod, common, torch, name, scenes, n_spheres, potentials, seed), seed
        except LookupError:
            continue
    return None, None


def main():
    stub_missing(["open3d", "torchvision.transforms.transforms", "natsort", "plyfile", "mayavi",
                  "cpp_wrappers.cpp_subsampling.grid_subsampling", "cpp_wrappers.cpp_neighbors.radius_neighbors"])
    sys.path.insert(0, REFROOT)
    import torch
    import datasets.common as common
    import datasets.ScanNet_sphere_color as mod
    scenes = make_scenes()
    for pot_seed in range(50):                        # both cases start from the SAME potentials
        potentials = [np.random.default_rng(1000 * pot_seed + i).random(len(s["pot_points"])) * 1e-3
                      for i, s in enumerate(scenes)]
        case2, seed2 = find_case(mod, common, torch, "stop2", scenes, 2, potentials)
        case3, seed3 = find_case(mod, common, torch, "stop3", scenes, 3, potentials) if case2 else (None, None)
        if case3:
            break
    else:
        raise SystemExit("no potentials in 50 served both cases")
    print("potentials seed %d; np.random seeds %d (stop2) and %d (stop3)" % (pot_seed, seed2, seed3))
    arrays = _Npz(header(scenes, potentials))
    arrays.update({"stop2/%s" % k: v for k, v in case2.items()})
    arrays.update({"stop3/%s" % k: v for k, v in case3.items()})
    for name in ("stop2", "stop3"):
        g = ref.golden_case(arrays, name)
        pots = [p.copy() for p in g["potentials"]]
        mine = ref.sphere_batch(g["scenes"], pots, g["config"], g["max_spheres"], int(g["batch_limit"]), NV, g["draws"], k=K,
                                noise=ref.golden_noise_rows(g))
        worst = ref.compare_with_golden(mine, g)
        for i, p in enumerate(pots):
            assert np.array_equal(p, g["potentials_after%d" % i]), "potentials of scene %d" % i
        print("%s: %d spheres of %s points, clouds %s, flips %s, symmetries %s, colours kept %s; the restatement reproduces "
              "every exact output; image_xyz differs by at most %.2f ulp of the largest coordinate"
              % (name, len(g["stack_lengths"]), g["stack_lengths"].tolist(), g["cloud_inds"].tolist(),
                 (g["flip_rand"] < FLIP).astype(int).tolist(), g["sym_rand"][:, 0].tolist(),
                 [d["keep_color"] for d in g["draws"]], worst))
    import sklearn
    arrays.update(numpy_version=np.array(np.__version__), sklearn_version=np.array(sklearn.__version__))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
