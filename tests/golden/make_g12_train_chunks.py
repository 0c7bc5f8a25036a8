#!/usr/bin/env python3
"""Generate tests/golden/g12_train_chunks.npz from the REFERENCE ITSELF (build container, CPU only).

Run from the repo root:   python tests/golden/make_g12_train_chunks.py

The reference's ScanNet2D3DChunks (mvpnet/data/scannet_2d3d.py) is imported from the reference tree at generation time
and its own __getitem__ is executed on a tiny synthetic cache (a pickle) and PNG / text frames written to a temporary
directory. Modules the reference imports but this container lacks (open3d, torchvision, ...) are stubbed in sys.modules:
none of them is reached with color_jitter=None. np.random's functions are wrapped so that every value the reference
draws is logged. Four cases (nb_pts 256, two views of 12 x 16, k 3):

  c0  a chunk with more than nb_pts points, flips and a rotation
  c1  a chunk with fewer than nb_pts points (a scene of 400 points): the pad branch
  c2  a first try that fails the threshold (half the scene is unlabeled), a rotation
  c3  the whole-scene fallback (nothing is labeled), flips

Per case, only arrays:
  inputs   points [n,3] f32, seg_label [n] int64 (training classes as the reference maps them), base_point_ind,
           overlap [nb,nf] bool, depth [nf,h,w] uint16, images [nf,h,w,3] f32 and poses [nf,4,4] f32 as the reference
           reads them back from the files, cam_matrix [3,3] f32 as it rescales it
  draws    centers [10] int64 (the centres it drew, -1 behind the last one), choice [nb_pts] int64 (crop_pad_choice),
           flips [nv] uint8, angle [1] f64 (nan: no rotation)
  outputs  points [3,nb_pts], seg_label, images [nv,3,h,w], image_xyz [nv,h,w,3], image_mask, knn_indices [nb_pts,k]
  derived  chunk_try, box [4] f32 and row (the chunk's point numbers) of tests/train_inputs_ref.py's crop fed the logged
           centres -- after this script has checked that the restatement fed the draws reproduces every output above

The generator re-draws its seed until the conditions hold that make an exact comparison fair: no pixel within 1e-6 of a
bound of the mask, no point within 1e-6 of an edge of the chosen box, the k+1 nearest distances of every query distinct
by more than 1e-9. It prints the largest difference between the reference's image_xyz and the restatement's (the two
evaluate the unprojection in different float orders); DESIGN.md 7q records it.

Only DATA is written; no reference source text.
"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g12_train_chunks.npz")
REFROOT = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_inputs_ref as ref  # noqa: E402

NB_PTS, NV, K, H, W, NF, TRIES = 256, 2, 3, 12, 16, 5, 10
SCALE = 40                                       # the reference rescales 640 x 480 intrinsics to 16 x 12
NYU40_OF_CLASS = None                            # filled from the reference's class list


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
    """Wraps np.random.randint / choice / rand / uniform and keeps what they returned."""

    def __init__(self):
        self.calls, self.saved = [], {}

    def __enter__(self):
        for name in ("randint", "choice", "rand", "uniform"):
            self.saved[name] = getattr(np.random, name)

            def wrapped(*a, _name=name, **kw):
                out = self.saved[_name](*a, **kw)
                self.calls.append((_name, a, kw, out))
                return out
            setattr(np.random, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(np.random, name, fn)


def write_scene(tmp, scan_id, scene, nyu40):
    from PIL import Image
    d = os.path.join(tmp, "images", scan_id)
    for sub in ("color", "depth", "pose"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    frame_ids = [str(100 + 7 * f) for f in range(NF)]
    for f, fid in enumerate(frame_ids):
        Image.fromarray(scene["color_u8"][f]).save(os.path.join(d, "color", fid + ".png"))
        Image.fromarray(scene["depth"][f].astype(np.uint16)).save(os.path.join(d, "depth", fid + ".png"))
        np.savetxt(os.path.join(d, "pose", fid + ".txt"), scene["poses"][f], fmt="%.9g")
    cam = np.eye(4, dtype=np.float64)
    cam[:3, :3] = scene["cam_matrix"].astype(np.float64)
    cam[0] *= SCALE
    cam[1] *= SCALE
    return {"scan_id": scan_id, "points": scene["points"].astype(np.float64), "seg_label": nyu40,
            "base_point_ind": scene["base_point_ind"].astype(np.int32), "pointwise_rgbd_overlap": scene["pointwise_rgbd_overlap"],
            "frame_ids": frame_ids, "cam_matrix": cam}


def make_scene(seed, n, labels):
    """labels: 'mixed' | 'half' | 'none'."""
    scene = ref.synthetic_scene(seed, n, nf=NF, nb=min(400, n // 2), h=H, w=W)
    rng = np.random.default_rng(seed + 7)
    scene["color_u8"] = rng.integers(0, 256, size=(NF, H, W, 3)).astype(np.uint8)
    scene["depth"] = scene["depth"].astype(np.uint16)
    cls = rng.integers(0, 20, n)
    nyu40 = NYU40_OF_CLASS[cls]
    if labels == "mixed":
        nyu40[rng.random(n) < 0.3] = 0
    elif labels == "half":
        nyu40[scene["points"][:, 0] < np.median(scene["points"][:, 0])] = 0     # 0 is no training class
        nyu40[rng.random(n) < 0.55] = 0
    else:
        nyu40[:] = 0
    return scene, nyu40.astype(np.int64)


def fair(scene_host, got):
    """The conditions of an exact comparison, on the restatement's own intermediate values."""
    lo_hi = got["box"].astype(np.float64)
    xy = scene_host["points"][:, :2].astype(np.float64)
    if got["chunk_try"] >= 0 and min(np.abs(xy[:, 0] - lo_hi[0]).min(), np.abs(xy[:, 0] - lo_hi[2]).min(),
                                    np.abs(xy[:, 1] - lo_hi[1]).min(), np.abs(xy[:, 1] - lo_hi[3]).min()) <= 1e-6:
        return "a point within 1e-6 of a box edge"
    b = ref.box_bounds(got["box"])
    keys = got["keys"]
    if min(np.abs(keys[:, 0] - b[0]).min(), np.abs(keys[:, 0] - b[1]).min(), np.abs(keys[:, 1] - b[2]).min(),
           np.abs(keys[:, 1] - b[3]).min()) <= 1e-6:
        return "a pixel within 1e-6 of a bound"
    valid = got["image_mask"].reshape(-1)
    if valid.sum() < K + 1:
        return "fewer than k + 1 valid pixels"
    q = np.ascontiguousarray(got["points_unrotated"]).astype(np.float64)
    kk = keys[valid]
    d = np.sqrt(((q[:, None, :] - kk[None, :, :]) ** 2).sum(-1))
    d.sort(axis=1)
    if np.diff(d[:, :K + 1], axis=1).min() <= 1e-9:
        return "two of the k + 1 nearest distances within 1e-9"
    return None


def run_case(mod, name, n, labels, want, flip, z_rot, seed0):
    """Runs the reference on one scene; re-draws the seed until `want` (a predicate on the logged draws and the
    restatement's result) and the fairness conditions hold. Returns the arrays of the case."""
    for seed in range(seed0, seed0 + 200):
        scene, nyu40 = make_scene(1000 + seed0, n, labels)
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "cache"))
            record = write_scene(tmp, "scene0000_00", scene, nyu40)
            with open(os.path.join(tmp, "cache", "scannetv2_train.pkl"), "wb") as f:
                pickle.dump([record], f)
            ds = mod.ScanNet2D3DChunks(os.path.join(tmp, "cache"), os.path.join(tmp, "images"), "train", nb_pts=NB_PTS,
                                       num_rgbd_frames=NV, resize=(W, H), k=K, z_rot=z_rot, flip=flip, to_tensor=True)
            np.random.seed(seed)
            try:
                with DrawLog() as log:
                    out = ds[0]
            except ValueError as e:                                  # scikit-learn: fewer valid pixels than k
                print("  %s seed %d: %s" % (name, seed, e))
                continue
            # the inputs as the reference saw them
            from PIL import Image
            d = os.path.join(tmp, "images", "scene0000_00")
            images = np.stack([np.asarray(Image.open(os.path.join(d, "color", fid + ".png")), dtype=np.float32) / 255.
                               for fid in record["frame_ids"]])
            depth = np.stack([np.asarray(Image.open(os.path.join(d, "depth", fid + ".png"))) for fid in record["frame_ids"]])
            poses = np.stack([np.loadtxt(os.path.join(d, "pose", fid + ".txt"), dtype=np.float32) for fid in record["frame_ids"]])
        assert np.array_equal(depth, scene["depth"]) and np.array_equal(poses, scene["poses"])
        cam = record["cam_matrix"].astype(np.float32)
        cam[0] /= SCALE
        cam[1] /= SCALE
        seg_label = ds.nyu40_to_scannet[nyu40].astype(np.int64)
        host = {"points": scene["points"], "seg_label": seg_label, "base_point_ind": scene["base_point_ind"].astype(np.int64),
                "pointwise_rgbd_overlap": scene["pointwise_rgbd_overlap"], "depth": depth.astype(np.uint16), "images": images,
                "poses": poses, "cam_matrix": cam[:3, :3].copy()}
        # the draws, in the reference's order: centres, the pad or the choice, a flip per view, the angle
        calls = list(log.calls)
        centers = []
        while calls and calls[0][0] == "randint" and not calls[0][2]:
            centers.append(int(calls.pop(0)[3]))
        kind, _, _, drawn = calls.pop(0)
        flips = np.zeros(NV, np.uint8)
        if flip:
            for v in range(NV):
                assert calls[0][0] == "rand"
                flips[v] = calls.pop(0)[3] < flip
        angle = float(calls.pop(0)[3]) if z_rot else float("nan")
        assert not calls and 1 <= len(centers) <= TRIES
        padded = np.full(TRIES, -1, np.int64)
        padded[:len(centers)] = centers
        probe = ref.crop(host["points"], seg_label, padded)
        nc = int(probe[3].sum())
        choice = np.hstack([np.arange(nc), drawn]) if kind == "randint" else np.asarray(drawn)
        assert (kind == "randint") == (nc < NB_PTS) and len(choice) == NB_PTS
        rot = None
        if z_rot:
            from scipy.spatial.transform import Rotation
            rot = Rotation.from_euler("z", angle, degrees=True).as_matrix()
        got = ref.item(host, padded, NB_PTS, NV, K, choice=choice, flips=flips if flip else None, rot=rot)
        got["points_unrotated"] = host["points"][got["row"][choice]]
        if not want(len(centers), got, nc):
            continue
        why = fair(host, got)
        if why:
            print("  %s seed %d: %s" % (name, seed, why))
            continue
        for key in ("points", "seg_label", "images", "image_mask", "knn_indices"):
            assert out[key].dtype == got[key].dtype and np.array_equal(out[key], got[key]), (name, key)
        diff = np.abs(out["image_xyz"].astype(np.float64) - got["image_xyz"].astype(np.float64))
        ulp = np.spacing(np.abs(got["image_xyz"]).astype(np.float32)).astype(np.float64)
        print("%s: seed %d, %d centre(s), try %d, %d chunk points, %d valid pixels, flips %s, angle %s; image_xyz differs "
              "by at most %.3g (%.2f ulp) in %d of %d values" % (name, seed, len(centers), got["chunk_try"], nc,
              got["num_valid_pixels"], flips.tolist(), angle, diff.max(), (diff / ulp).max(), (diff > 0).sum(), diff.size))
        case = {k: host[k] for k in host}
        case["overlap"] = case.pop("pointwise_rgbd_overlap")
        case.update(centers=padded, choice=choice.astype(np.int64), flips=flips, angle=np.array([angle]),
                    out_points=out["points"], out_seg_label=out["seg_label"], out_images=out["images"],
                    out_image_xyz=out["image_xyz"], out_image_mask=out["image_mask"], out_knn_indices=out["knn_indices"],
                    chunk_try=np.array([got["chunk_try"]], np.int32), box=got["box"], row=got["row"].astype(np.int64))
        return {"%s/%s" % (name, k): v for k, v in case.items()}
    raise SystemExit("%s: no seed in 200 satisfied the case's conditions" % name)


def main():
    global NYU40_OF_CLASS
    stub_missing(["open3d", "torchvision.transforms.transforms", "torchvision.transforms.functional", "natsort", "tqdm"])
    sys.path.insert(0, REFROOT)
    import mvpnet.data.scannet_2d3d as mod
    from mvpnet.data.scannet_2d import load_class_mapping
    NYU40_OF_CLASS = np.array(list(load_class_mapping(mod.ScanNet2D3DChunks.scannet_classes_path).keys()), np.int64)
    assert len(NYU40_OF_CLASS) == 20
    arrays = {}
    arrays.update(run_case(mod, "c0", 3000, "mixed", lambda nt, got, nc: nt == 1 and nc > NB_PTS, 0.5, (-180, 180), 10))
    arrays.update(run_case(mod, "c1", 400, "mixed", lambda nt, got, nc: nc < NB_PTS and got["chunk_try"] >= 0, 0.0, None, 20))
    arrays.update(run_case(mod, "c2", 3000, "half", lambda nt, got, nc: 2 <= nt < TRIES and got["chunk_try"] == nt - 1
                           and got["counts"][0, 0] > 0, 0.0, (-180, 180), 30))
    arrays.update(run_case(mod, "c3", 3000, "none", lambda nt, got, nc: nt == TRIES and got["chunk_try"] == -1, 0.5, None, 40))
    import sklearn
    arrays.update(numpy_version=np.array(np.__version__), sklearn_version=np.array(sklearn.__version__),
                  nb_pts=np.array(NB_PTS), nv=np.array(NV), k=np.array(K))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
