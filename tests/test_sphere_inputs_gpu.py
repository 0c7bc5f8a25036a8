"""GPU: the sphere batches of the KPFCNN networks built on the device from resident scenes (csrc/sphere_inputs.hip,
dropin/datasets/sphere_inputs.py). Every stage against what the library already had for ONE sphere at a time -- the picks
against PotentialSphereSampler.pick(), the rows against ops.ball_query, the frame choice against voting.select_frames, the
unprojection against ops.unproject_depth -- and against the NumPy restatement (tests/sphere_inputs_ref.py); the whole
batch against the restatement and against the reference's own potential_item (fixture g18, fed its logged draws); the
batch through the drop-in's early-fusion KPFCNN_featureAggre and baseline KPFCNN forward and backward; and no wait for
the device. Integers compare equal, floats compare as bits; image_xyz against the reference's float order is held to 2
float32 ulp of the largest coordinate (DESIGN.md 7q's bound)."""
import itertools
import os

import numpy as np
import pytest
import torch

import sphere_inputs_ref as ref
from util import check_err

pytestmark = pytest.mark.gpu

R_IN, MARGIN, NV = 0.8, 0.1, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_sphere_batch.npz")


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def si():
    import mvkpconv
    return mvkpconv.sub("dropin.datasets.sphere_inputs")


@pytest.fixture(scope="module")
def dropin():
    import mvkpconv
    return mvkpconv.sub


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same(got, want):
    """A device tensor and a host array of one shape and dtype with the same bytes."""
    got, want = host(got), np.asarray(want)
    if got.dtype == np.bool_ or want.dtype == np.bool_:
        got, want = got.astype(np.uint8), want.astype(np.uint8)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(
        np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def on_device(scene):
    d = {key: dev(scene[key]) for key in ("points", "colors", "labels", "pot_points", "images", "poses", "base_point_ind",
                                          "pointwise_rgbd_overlap")}
    d["depth"] = dev(np.asarray(scene["depth"]).astype(np.uint16).view(np.int16))
    d["cam_matrix"] = scene["cam_matrix"]
    return d


def make_world(si, scenes, seed=9, in_radius=R_IN):
    pots = [np.random.default_rng(seed + i).random(len(s["pot_points"])) * 1e-3 for i, s in enumerate(scenes)]
    ss = si.SphereScenes([on_device(s) for s in scenes], in_radius, MARGIN, init_potentials=[p.copy() for p in pots])
    offs = np.concatenate([[0], np.cumsum([len(s["points"]) for s in scenes])])
    return dict(scenes=scenes, ss=ss, pots=pots, point_off=offs)


def world_scenes():
    """Four scenes around the 1 024-point tile. Scene 3's base points all lie at x > 2.4: a sphere at the other end of the
    room has none."""
    scenes = [ref.synthetic_scene(1, 1023, nf=5), ref.synthetic_scene(2, 2500), ref.synthetic_scene(3, 1025, nf=7),
              ref.synthetic_scene(4, 3000)]
    s3 = scenes[3]
    far = np.nonzero(s3["points"][:, 0] > 2.4)[0]
    s3["base_point_ind"] = np.sort(far[:len(s3["base_point_ind"])]).astype(np.int64)
    s3["pointwise_rgbd_overlap"] = s3["pointwise_rgbd_overlap"][:len(s3["base_point_ind"])]
    return scenes


@pytest.fixture(scope="module")
def world(si):
    return make_world(si, world_scenes())


class Cfg(object):
    in_radius = R_IN
    augment_rotation = 'vertical'
    augment_scale_min, augment_scale_max = 0.9, 1.1
    augment_scale_anisotropic = True
    augment_symmetries = [True, False, False]
    augment_color = 0.7
    early_fusion = True
    in_features_dim = 66


# ------------------------------------------------------------------------------------------------------------ the picks

def batch_limit_for(scenes, pots, stop_at, max_spheres):
    """A limit that the running sum of the restatement's sphere sizes exceeds first at slot stop_at (None: never)."""
    slots = ref.pick(scenes, [p.copy() for p in pots], R_IN, 1 << 40, max_spheres)
    sums = np.cumsum([len(s["input_inds"]) for s in slots])
    return int(sums[-1]) + 5 if stop_at is None else int(sums[stop_at]) - 1


@pytest.mark.parametrize("stop_at", [0, 2, 4, None])
def test_pick_equals_the_one_sphere_sampler(ops, si, dropin, stop_at):
    """B_max = 5 picks in one launch against five calls of PotentialSphereSampler.pick() from the same potentials: the
    same clouds, points and centres, the stop rule at the first, a middle and the last slot or never, and bit-equal
    potentials afterwards. Two scenes: several picks fall into one scene."""
    scenes = world_scenes()[:2]
    w = make_world(si, scenes, seed=30)
    limit = batch_limit_for(scenes, w["pots"], stop_at, 5)
    sampler = dropin("dropin.datasets.sphere_picking").PotentialSphereSampler(
        [s["pot_points"] for s in scenes], [s["points"] for s in scenes], R_IN, MARGIN, init_potentials=[p.copy() for p in w["pots"]])
    want, batch_n = [], 0
    for _ in range(5):
        p = sampler.pick()
        want.append(p)
        batch_n += p["input_inds"].shape[0]
        if batch_n > limit:
            break
    n = len(want)
    assert n == (5 if stop_at is None else stop_at + 1)
    cloud, point, centers, lengths, num = ops.sphere_pick(w["ss"].sphere, R_IN, limit, 5)
    assert int(num.item()) == n
    assert host(cloud).tolist() == [p["cloud_ind"] for p in want] + [-1] * (5 - n)
    assert host(point).tolist() == [p["point_ind"] for p in want] + [-1] * (5 - n)
    assert host(lengths).tolist() == [p["input_inds"].shape[0] for p in want] + [0] * (5 - n)
    assert same(centers[:n], np.stack([p["center"] for p in want]).astype(np.float32))
    assert (host(centers[n:]) == 0).all()
    assert len({p["cloud_ind"] for p in want}) < n or n == 1              # two picks in one scene
    for s in range(2):
        assert same(w["ss"].potentials(s), host(sampler.potentials[s])), "potentials of scene %d" % s
    assert same(w["ss"].sphere.min_potentials, host(sampler.min_potentials))
    assert host(w["ss"].sphere.argmin_potentials).tolist() == host(sampler.argmin_potentials).tolist()
    # and the restatement
    slots = ref.pick(scenes, [p.copy() for p in w["pots"]], R_IN, limit, 5)
    assert [s["cloud_ind"] for s in slots] == host(cloud)[:n].tolist()


# ------------------------------------------------------------------------------------------------------------- the rows

def test_members_equal_ball_query_around_the_tile(ops, world):
    """Every scene whole (1 023, 2 500, 1 025, 3 000 points: below, above and across the 1 024-point tile), small spheres,
    a slot of no scene, and a point exactly on the bound."""
    scenes, res = world["scenes"], world["ss"].resident
    pts1 = scenes[1]["points"]
    centre_on = pts1[7].astype(np.float64) - np.array([0.5, 0.0, 0.0])     # point 7 lies at distance 0.5 exactly ...
    centre_on = centre_on.astype(np.float32)
    assert ((pts1[7].astype(np.float64) - centre_on.astype(np.float64)) ** 2).sum() == 0.25
    for radius, ids, centers in ((10.0, [0, 1, 2, 3, -1, 7], None), (0.5, [1, 3, 0, 1, 2], None), (0.5, [1, 1], [centre_on, pts1[99]])):
        if centers is None:
            centers = [scenes[s]["points"][11 * (b + 1)] if 0 <= s < 4 else np.zeros(3, np.float32) for b, s in enumerate(ids)]
        want = [host(ops.ball_query(dev(scenes[s]["points"]), c.astype(np.float64), radius)) + world["point_off"][s]
                if 0 <= s < 4 else np.zeros(0, np.int64) for s, c in zip(ids, centers)]
        q = np.concatenate([[0], np.cumsum([len(v) for v in want])])
        rows, q_off, status = ops.sphere_members(res, dev(np.asarray(ids, np.int64)), dev(np.stack(centers).astype(np.float32)),
                                                 radius, int(q[-1]) + 9)
        assert host(q_off).tolist() == q.tolist() and host(status).tolist() == [0]
        assert np.array_equal(host(rows)[:q[-1]], np.concatenate(want))
        if radius == 10.0:
            assert (np.diff(q) == [1023, 2500, 1025, 3000, 0, 0]).all()
    assert world["point_off"][1] + 7 in np.concatenate(want)               # ... and is a member: rdist <= r^2


def test_members_that_do_not_fit_cap_are_dropped_and_reported(ops, world):
    scenes, res = world["scenes"], world["ss"].resident
    ids = [0, 1, 2]
    centers = np.stack([scenes[s]["points"][0] for s in ids])
    full, q_full, _ = ops.sphere_members(res, dev(np.asarray(ids, np.int64)), dev(centers), 10.0, 5000)
    cap = 1023 + 1500                                                       # slot 1 is cut, slot 2 gets nothing
    rows, q_off, status = ops.sphere_members(res, dev(np.asarray(ids, np.int64)), dev(centers), 10.0, cap)
    assert host(q_off).tolist() == [0, 1023, cap, cap] and host(status).tolist() == [1]
    assert rows.shape[0] == cap and torch.equal(rows, full[:cap])


# ----------------------------------------------------------------------------------------------------- the frame choice

def test_frame_choice_equals_select_frames_on_the_mask_sphere(ops, dropin, world):
    """Per slot, voting.select_frames on the overlap rows of the base points inside the mask sphere (found with
    ops.ball_query); a sphere without a base point and a slot of no scene choose frame 0."""
    voting = dropin("dropin.utils.voting")
    scenes, res = world["scenes"], world["ss"].resident
    ids = [0, 1, 2, 3, 3, -1]
    s3 = scenes[3]
    centers = [scenes[s]["points"][5] for s in ids[:3]] + [s3["points"][s3["base_point_ind"][0]]]
    centers += [s3["points"][np.argmin(s3["points"][:, 0])], np.zeros(3, np.float32)]      # no base point within 0.9 m
    cloud, cen = dev(np.asarray(ids, np.int64)), dev(np.stack(centers).astype(np.float32))
    mask_rows, mask_off, status = ops.sphere_members(res, cloud, cen, R_IN + MARGIN, 6000)
    sel = host(ops.sphere_select_frames(res, cloud, mask_rows, mask_off, NV))
    assert host(status).tolist() == [0]
    for b, s in enumerate(ids):
        if s < 0:
            want = [0] * NV
        else:
            inside = host(ops.ball_query(dev(scenes[s]["points"]), centers[b].astype(np.float64), R_IN + MARGIN))
            rows = scenes[s]["pointwise_rgbd_overlap"][np.isin(scenes[s]["base_point_ind"], inside)]
            want = voting.select_frames(rows, NV)
            assert (len(rows) == 0) == (b == 4)
            assert want == ref.select_frames(scenes[s]["pointwise_rgbd_overlap"], scenes[s]["base_point_ind"], inside, NV)
        assert sel[b].tolist() == want, "slot %d" % b


# ------------------------------------------------------------------------------------------------------ the unprojection

def reference_order_xyz(cam_matrix, pose, depth_mm):
    """The reference's float order (ScanNet_sphere_color.py:66-72, :410-417): float32 depth in metres, the float32 inverse
    of the intrinsics times int64 pixel coordinates, times the depth, then a matmul with the float32 pose."""
    depth = np.asarray(depth_mm.astype(np.uint16), dtype=np.float32) / 1000.
    v, u = np.indices(depth.shape)
    uv1 = np.stack([u.ravel(), v.ravel(), np.ones_like(u.ravel())], axis=1)
    xyz = (np.linalg.inv(cam_matrix[:3, :3]).dot(uv1.T) * depth.ravel()).T
    return (np.matmul(xyz, pose[:3, :3].T) + pose[:3, 3]).reshape(depth.shape + (3,)), (xyz[:, 2] > 0).reshape(depth.shape)


@pytest.mark.parametrize("flips", list(itertools.product([0, 1], repeat=2)))
def test_unprojection_for_every_flip_pattern(ops, world, flips):
    """nv = 2: frame 1 of every scene has no depth at all. Exact against the restatement and against ops.unproject_depth
    (mirrored on the host); image_xyz within 2 float32 ulp of the largest coordinate of the reference's own float order."""
    scenes, res = world["scenes"], world["ss"].resident
    ids, sel = [0, 2, -1, 3], np.array([[1, 3], [6, 1], [0, 0], [2, 11]], np.int32)
    fl = np.tile(np.asarray(flips, np.uint8), (4, 1))
    keys, image_xyz, image_mask, images, num_valid = ops.sphere_unproject(res, dev(sel), dev(np.asarray(ids, np.int64)), flips=dev(fl))
    worst = 0.0
    for b, s in enumerate(ids):
        if s < 0:
            assert not host(image_mask[b]).any() and (host(keys[b]) == 0).all() and (host(images[b]) == 0).all()
            continue
        want_img, want_keys, want_mask = ref.views(scenes[s], sel[b], fl[b])
        assert same(keys[b], want_keys) and same(image_mask[b], want_mask)
        assert same(image_xyz[b], want_keys.astype(np.float32).reshape(want_mask.shape + (3,)))
        assert same(images[b], np.moveaxis(want_img, -1, 1))
        assert int(num_valid[b].item()) == want_mask.sum()
        sc = scenes[s]
        xyz, valid = ops.unproject_depth(dev(sc["depth"][sel[b]].view(np.int16)), sc["cam_matrix"], dev(sc["poses"][sel[b]]))
        xyz, valid = host(xyz), host(valid)
        for v in range(2):
            x, ok = (np.fliplr(xyz[v]), np.fliplr(valid[v])) if fl[b, v] else (xyz[v], valid[v])
            assert np.array_equal(host(keys[b]).reshape(2, sc["depth"].shape[1], -1, 3)[v], x)
            assert np.array_equal(host(image_mask[b][v]), ok)
            theirs, their_ok = reference_order_xyz(sc["cam_matrix"], sc["poses"][sel[b, v]], sc["depth"][sel[b, v]])
            if fl[b, v]:
                theirs, their_ok = np.fliplr(theirs), np.fliplr(their_ok)
            assert np.array_equal(their_ok, ok)
            mine = host(image_xyz[b][v]).astype(np.float64)
            ulp = float(np.spacing(np.float32(np.abs(theirs).max())))
            worst = max(worst, np.abs(mine - theirs.astype(np.float32)).max() / ulp)
        for v in range(2):
            if sel[b, v] == 1:                                              # the frame without depth
                assert not host(image_mask[b][v]).any()
    check_err("sphere image_xyz vs the reference's float order, flips %s [ulp of the largest coordinate]" % (flips,), worst, 2.0 + 1e-9)


# -------------------------------------------------------------------------------------------------------- the batch rows

@pytest.mark.parametrize("with_noise", [False, True])
def test_batch_rows(ops, world, with_noise):
    """Centring, augmentation in the reference's float32 order, the features' columns, labels, scene-local indices and the
    stacked k-NN; a colour drop in slot 1; a slot of no scene; rows behind the total; a row outside its scene."""
    scenes, ss = world["scenes"], world["ss"]
    rng = np.random.default_rng(3 + with_noise)
    ids = [1, 3, -1, 0]
    centers = np.stack([scenes[s]["points"][3] if s >= 0 else np.zeros(3, np.float32) for s in ids]).astype(np.float32)
    cloud, cen = dev(np.asarray(ids, np.int64)), dev(centers)
    rows, q_off, _ = ops.sphere_members(ss.resident, cloud, cen, R_IN, 2000)
    rows_h, q = host(rows).copy(), host(q_off)
    total, cap = int(q[-1]), 2000
    assert 0 < total < cap - 10
    rows_h[q[1] + 2] = world["point_off"][0]                                # a point of another scene in slot 1
    rows_h[total:] = 0
    draws = [dict(rot=rng.random(1), scale=rng.random(3), sym=rng.integers(0, 2, 3)) for _ in ids]
    aug = [ref.augment_params(Cfg, d) for d in draws]
    R, scale = np.stack([a[0] for a in aug]), np.stack([a[1] for a in aug])
    keep = np.array([1, 0, 1, 1], np.float32)
    noise = (rng.standard_normal((cap, 3)) * 0.005).astype(np.float32) if with_noise else None
    npix, k = 3 * 12 * 16, 3
    knn = rng.integers(-1, npix, (cap, k)).astype(np.int64)
    out = ops.sphere_batch_rows(ss.sphere, cloud, cen, dev(rows_h), q_off, dev(R.reshape(4, 9)), dev(scale), dev(keep), dev(knn),
                                npix, noise=None if noise is None else dev(noise))
    want = {key: np.zeros((cap, 3), np.float32) for key in ("points", "world", "feat_aggre_points", "colors")}
    want.update(labels=np.zeros(cap, np.int64), input_inds=np.full(cap, -1, np.int64), knn_stacked=np.full((cap, k), -1, np.int64))
    for b, s in enumerate(ids):
        for i in range(q[b], q[b + 1]):
            r = rows_h[i] - world["point_off"][s]
            if s < 0 or not 0 <= r < len(scenes[s]["points"]):
                continue
            p = scenes[s]["points"][r:r + 1]
            x = (p.astype(np.float64) - centers[b].astype(np.float64)).astype(np.float32)
            a = ref.augment(x, R[b], scale[b], None if noise is None else noise[i:i + 1])
            want["points"][i], want["feat_aggre_points"][i] = a[0], p[0]
            want["world"][i] = (a.astype(np.float64) + centers[b].astype(np.float64)).astype(np.float32)[0]
            want["colors"][i] = scenes[s]["colors"][r] * keep[b]
            want["labels"][i], want["input_inds"][i] = scenes[s]["labels"][r], r
            want["knn_stacked"][i] = np.where(knn[i] >= 0, knn[i] + b * npix, -1)
    assert want["input_inds"][q[1] + 2] == -1 and (want["colors"][q[1]:q[2]] == 0).all() and want["colors"][:q[1]].any()
    for key in want:
        assert same(out[key], want[key]), key


# -------------------------------------------------------------------------------------------------------- the whole batch

def draws_for(rng, B, flip=True):
    return [dict(flip=(rng.random(NV) < 0.5) if flip else None, rot=rng.random(1), scale=rng.random(3),
                 sym=rng.integers(0, 2, 3), keep_color=bool(rng.random() <= 0.7)) for _ in range(B)]


def compare_batch(out, want, cap, B):
    n, total = want["num_spheres"], len(want["points"])
    assert int(out["num_spheres"].item()) == n and host(out["status"]).tolist() == [0, 0]
    assert host(out["stack_lengths"]).tolist() == want["stack_lengths"].tolist() + [0] * (B - n)
    assert host(out["cloud_inds"]).tolist() == want["cloud_inds"].tolist() + [-1] * (B - n)
    assert host(out["point_inds"]).tolist() == want["point_inds"].tolist() + [-1] * (B - n)
    for key in ("points", "labels", "input_inds", "features", "feat_aggre_points", "knn", "knn_stacked"):
        assert same(out[key][:total], want[key]), key
        tail = host(out[key][total:])
        assert ((tail == -1) if key in ("input_inds", "knn", "knn_stacked") else (tail[:, 1:] == 0) if key == "features"
                else (tail == 0)).all(), key
    for key in ("images", "image_xyz", "image_mask", "centers"):
        assert same(out[key][:n], want[key]), key
    assert same(out["scales"][:n], want["scales"]) and same(out["rots"][:n], want["rots"])
    assert host(out["sel"][:n]).tolist() == want["sel"].tolist() and (host(out["sel"][n:]) == 0).all()


@pytest.mark.parametrize("limit, with_noise", [(700, False), (1 << 30, True)])
def test_sphere_batch_equals_the_restatement(si, world, limit, with_noise):
    """Two batches in a row from the same resident potentials (the second starts where the first left them), stopped by
    batch_limit and by max_spheres, with flips, a symmetry, colour drops and noise."""
    scenes = world["scenes"]
    w = make_world(si, scenes, seed=50 + with_noise)
    pots = [p.copy() for p in w["pots"]]
    rng = np.random.default_rng(limit % 97)
    B, cap = 4, 2600
    for _ in range(2):
        draws = draws_for(rng, B)
        noise = (rng.standard_normal((cap, 3)) * 0.005).astype(np.float32) if with_noise else None
        out = si.sphere_batch(w["ss"], Cfg, B, limit, cap, NV, k=3, noise=None if noise is None else dev(noise), draws=draws)
        want = ref.sphere_batch(scenes, pots, Cfg, B, limit, NV, draws, k=3, mask_margin=MARGIN, noise=noise)
        assert want["num_spheres"] == (B if with_noise else want["num_spheres"]) and want["num_spheres"] >= 2
        compare_batch(out, want, cap, B)
        for s in range(len(scenes)):
            assert same(w["ss"].potentials(s), pots[s])


@pytest.mark.parametrize("case", ["stop2", "stop3"])
def test_sphere_batch_equals_the_reference_fed_its_draws(si, case):
    """The reference's own potential_item (fixture g18): the same spheres, and per sphere -- after sorting both by
    input_inds, the reference's order being its KD-tree's -- the same points, features, labels, k-NN, images and masks."""
    g = ref.golden_case(np.load(GOLDEN), case)
    scenes, cfg = g["scenes"], g["config"]
    ss = si.SphereScenes([on_device(s) for s in scenes], cfg.in_radius, 0.1, init_potentials=[p.copy() for p in g["potentials"]])
    B, cap = int(g["max_spheres"]), 4000
    out = si.sphere_batch(ss, cfg, B, int(g["batch_limit"]), cap, int(g["nv"]), k=int(g["k"]), draws=g["draws"],
                          noise=dev(ref.golden_noise_rows(g, cap)))
    ref.compare_with_golden({key: host(v) for key, v in out.items()}, g)


# ----------------------------------------------------------------------------------------------------------- the networks

@pytest.mark.parametrize("variant", ["early", "baseline"])
def test_batch_through_the_networks_forward_and_backward(si, dropin, variant):
    syn = dropin("synthetic")
    cfg = syn.make_config(variant)
    cfg.architecture = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'nearest_upsample', 'unary']
    cfg.first_features_dim, cfg.first_subsampling_dl, cfg.in_radius = 16, 0.1, R_IN
    cfg.augment_symmetries = [True, False, False]
    scenes = [ref.synthetic_scene(21, 1500, nf=4, h=24, w=32), ref.synthetic_scene(22, 1700, nf=4, h=24, w=32)]
    w = make_world(si, scenes, seed=70)
    np.random.seed(11)
    out = si.sphere_batch(w["ss"], cfg, 3, 600, 2000, 2, k=3, flip=0.5)
    batch = si.to_sphere_batch(out, cfg)
    n = int(out["num_spheres"].item())
    assert 2 <= n <= 3 and sum(int(v) for v in batch.lengths[0]) == batch.points[0].shape[0] == batch.labels.shape[0]
    torch.manual_seed(0)
    net = syn.build_model(cfg, torch.device("cuda:0"))
    net.train()
    if variant == "early":
        for m in net.net_2d._modules.values():
            m.train(False)
    logits = net(batch, cfg)
    loss = net.loss(logits, batch.labels)
    loss.backward()
    assert torch.isfinite(loss).item() and logits.shape == (batch.labels.shape[0], cfg.num_classes)
    grads = [p.grad for p in net.parameters() if p.requires_grad and p.grad is not None]
    assert grads and all(torch.isfinite(g).all().item() for g in grads)


def test_to_sphere_batch_reports_overflow_and_too_few_pixels(si, world):
    scenes = world["scenes"]
    w = make_world(si, scenes, seed=80)
    out = si.sphere_batch(w["ss"], Cfg, 3, 1 << 30, 300, NV, draws=draws_for(np.random.default_rng(1), 3))
    assert host(out["status"])[0] == 1
    with pytest.raises(ValueError, match="did not fit"):
        si.to_sphere_batch(out, Cfg)
    dark = [dict(s, depth=np.zeros_like(s["depth"])) for s in scenes[:2]]
    w = make_world(si, dark, seed=81)
    out = si.sphere_batch(w["ss"], Cfg, 2, 1 << 30, 3000, NV, draws=draws_for(np.random.default_rng(2), 2))
    assert (host(out["knn"]) == -1).all() and host(out["num_valid_pixels"]).tolist() == [0, 0]
    with pytest.raises(ValueError, match="Expected n_neighbors <= n_samples"):
        si.to_sphere_batch(out, Cfg)


def test_sphere_batch_never_waits_for_the_device(si, world):
    w = make_world(si, world["scenes"], seed=90)

    def batches():
        np.random.seed(5)
        return [si.sphere_batch(w["ss"], Cfg, 4, 900, 2600, NV, k=3, flip=0.5), si.sphere_batch(w["ss"], Cfg, 2, 1 << 30, 2600, 1, k=1)]

    batches()                                                           # first use: allocations, the workspace
    torch.cuda.synchronize()
    one = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            one.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            got = batches()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error')")
    assert all(int(g["num_spheres"].item()) >= 1 for g in got)


def test_cpu_tensors_and_bad_sizes_are_refused(ops, world):
    res, sres = world["ss"].resident, world["ss"].sphere
    cloud, cen = dev(np.zeros(2, np.int64)), dev(np.zeros((2, 3), np.float32))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.sphere_members(res, cloud.cpu(), cen, 0.5, 10)
    with pytest.raises(RuntimeError, match="centers"):
        ops.sphere_members(res, cloud, cen[:1], 0.5, 10)
    with pytest.raises(RuntimeError, match="SphereResident"):
        ops.sphere_pick(res, 0.5, 10, 2)
    with pytest.raises(RuntimeError, match="slots"):
        ops.sphere_pick(sres, 0.5, 10, 5000)
    with pytest.raises(RuntimeError, match="mask_off"):
        ops.sphere_select_frames(res, cloud, dev(np.zeros(4, np.int64)), dev(np.zeros(2, np.int64)), 2)
